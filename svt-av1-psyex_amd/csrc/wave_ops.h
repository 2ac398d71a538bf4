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

// maximum: the same steps as wave_min_dpp.  A lane the step does not write takes 0, the identity of the unsigned maximum: with that the step is
// one v_max_u32 with a DPP operand (with `v` itself as the old value it is a copy, a v_mov_b32_dpp and the maximum)
template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t dpp_max_step(uint32_t v) {
    const uint32_t t = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, ROWS == 0xF);
    return t > v ? t : v;
}
__device__ __forceinline__ uint32_t wave_max_dpp(uint32_t v) {
    v = dpp_max_step<0xB1, 0xF>(v);  // quad_perm [1,0,3,2]
    v = dpp_max_step<0x4E, 0xF>(v);  // quad_perm [2,3,0,1]
    v = dpp_max_step<0x141, 0xF>(v); // row_half_mirror
    v = dpp_max_step<0x140, 0xF>(v); // row_mirror
    v = dpp_max_step<0x142, 0xA>(v); // row_bcast:15 -> rows 1, 3
    v = dpp_max_step<0x143, 0xC>(v); // row_bcast:31 -> rows 2, 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// ---- DPP forms over a part of the wave, the result in all of its lanes
// group_sum_dpp<G> / group_max_dpp<G>: what group_sum<G> / group_max<G> return, for G = 4 .. 64 consecutive lanes, EVERY lane of the wave
// active.  Inside a 16-lane row the steps are DPP operands of the additions themselves; a group of 32 or 64 lanes then takes its rows' results
// (uniform inside each row) from one lane per row through scalar registers.
template <int G> __device__ __forceinline__ uint32_t group_sum_dpp(uint32_t v) {
    static_assert(G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "a quad, half a row, a row, two rows or the wave");
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, true);
    if constexpr (G >= 8) v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x141 /* row_half_mirror */, 0xF, 0xF, true);
    if constexpr (G >= 16) v += (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x140 /* row_mirror */, 0xF, 0xF, true);
    if constexpr (G >= 32) {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
        const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
        if constexpr (G == 64) v = r0 + r1 + r2 + r3;
        else v = threadIdx.x < 32 ? r0 + r1 : r2 + r3; // (callers are one-wave workgroups)
    }
    return v;
}
template <int G> __device__ __forceinline__ uint32_t group_max_dpp(uint32_t v) {
    static_assert(G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "a quad, half a row, a row, two rows or the wave");
    v = dpp_max_step<0xB1, 0xF>(v);
    v = dpp_max_step<0x4E, 0xF>(v);
    if constexpr (G >= 8) v = dpp_max_step<0x141, 0xF>(v);
    if constexpr (G >= 16) v = dpp_max_step<0x140, 0xF>(v);
    if constexpr (G >= 32) {
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
        const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
        const uint32_t m01 = r0 > r1 ? r0 : r1, m23 = r2 > r3 ? r2 : r3;
        if constexpr (G == 64) v = m01 > m23 ? m01 : m23;
        else v = threadIdx.x < 32 ? m01 : m23;
    }
    return v;
}
// the 64-bit sum of a group's 32-bit values (a lane's own sum fits 32 bits, the group's may not): the two 16-bit halves are summed apart, each
// below G * 2^16, and joined afterwards
template <int G> __device__ __forceinline__ uint64_t group_sum_wide_dpp(uint32_t v) {
    const uint64_t lo = group_sum_dpp<G>(v & 0xFFFFu), hi = group_sum_dpp<G>(v >> 16);
    return (hi << 16) + lo;
}
// a 64-bit sum (mod 2^64) of values below 2^BITS, in pieces of 32 - log2(G) bits: none of them can overflow its 32-bit sum over G lanes
template <int G, int BITS = 64> __device__ __forceinline__ uint64_t group_sum64_dpp(uint64_t v) {
    constexpr int P = 32 - (G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6);
    uint64_t s = 0;
#pragma unroll
    for (int b = 0; b < BITS; b += P) s += (uint64_t)group_sum_dpp<G>((uint32_t)(v >> b) & ((1u << P) - 1u)) << b;
    return s;
}
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
