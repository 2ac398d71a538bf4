// txfm_pass_isa.hip -- one bounded 1-D transform pass per lane (txfm_core.h), with the round-shift that follows it in rd_tx_kernel, as kernels of
// their own: what the compiler makes of a pass can be counted without the rest of the RD kernel around it.  Not meant to be run.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I svt-av1-psyex_amd/csrc tools/ubench/txfm_pass_isa.hip -o pass.s
// -DTXFM_PASS_UNFOLDED builds the pass and the shift loop apart (fwd_1d<N, 2> / inv_1d<N, C, 2>, then shift_vec), which also compiles
// against an older txfm_core.h.  The counts of profiles/r07_rd_butterfly_before_after.txt are of these kernels.
#include <hip/hip_runtime.h>
#include "txfm_core.h"

template <int N, int BIT, int SH, bool SAFE32> __global__ void fwd_dct_pass(const int32_t *in, int32_t *out) {
    int32_t x[N];
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = in[(size_t)i * 64 + threadIdx.x];
#ifdef TXFM_PASS_UNFOLDED
    fwd_1d<N, 2>(x, 0, BIT);
    shift_vec<N, SAFE32>(x, SH);
#else
    fwd_1d_bounded<N, SAFE32>(x, 0, BIT, SH);
#endif
#pragma unroll
    for (int i = 0; i < N; i++) out[(size_t)i * 64 + threadIdx.x] = x[i];
}
// NZ: leading inputs that are not literal zeros (32 of 64 in the 64-point passes of rd_tx_kernel)
template <int N, int NZ, int CLAMP, int SH, bool SAFE32> __global__ void inv_dct_pass(const int32_t *in, int32_t *out) {
    int32_t x[N];
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = i < NZ ? in[(size_t)i * 64 + threadIdx.x] : 0;
#ifdef TXFM_PASS_UNFOLDED
    inv_1d<N, CLAMP, 2>(x, 0);
    shift_vec<N, SAFE32>(x, SH);
#else
    inv_1d_bounded<N, CLAMP, SAFE32, true>(x, 0, SH);
#endif
#pragma unroll
    for (int i = 0; i < N; i++) out[(size_t)i * 64 + threadIdx.x] = x[i];
}
// the passes of the three sizes the benchmark runs (TX_16X16, TX_32X32, TX_64X64 at 10 bits): columns then rows
template __global__ void fwd_dct_pass<16, 13, -2, true>(const int32_t *, int32_t *);
template __global__ void fwd_dct_pass<16, 12, 0, true>(const int32_t *, int32_t *);
template __global__ void fwd_dct_pass<32, 12, -4, false>(const int32_t *, int32_t *);
template __global__ void fwd_dct_pass<32, 12, 0, false>(const int32_t *, int32_t *);
template __global__ void fwd_dct_pass<64, 13, -2, true>(const int32_t *, int32_t *);
template __global__ void fwd_dct_pass<64, 10, -2, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<16, 16, 18, -2, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<16, 16, 16, -4, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<32, 32, 18, -2, false>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<32, 32, 16, -4, false>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<64, 32, 18, -2, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<64, 32, 16, -4, true>(const int32_t *, int32_t *);
// the same six inverse passes in the clamp-free tier (CLAMP < 0: ipass_clamp_free holds for the wave), rows (-2) then columns (-4)
template __global__ void inv_dct_pass<16, 16, -1, -2, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<16, 16, -1, -4, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<32, 32, -1, -2, false>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<32, 32, -1, -4, false>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<64, 32, -1, -2, true>(const int32_t *, int32_t *);
template __global__ void inv_dct_pass<64, 32, -1, -4, true>(const int32_t *, int32_t *);
