// tx_geom.h -- the geometry of the 19 AV1 transform sizes as compile-time functions of TxSize, for host and device: nothing else, so a
// translation unit that only needs a width does not get the constant tables of txfm_core.h.
#ifndef SVT_HIP_TX_GEOM_H
#define SVT_HIP_TX_GEOM_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ constexpr int tx_wide(int s) { constexpr uint8_t t[19] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64}; return t[s]; }
__host__ __device__ constexpr int tx_high(int s) { constexpr uint8_t t[19] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16}; return t[s]; }
__host__ __device__ constexpr int ilog2c(int n) { return n <= 1 ? 0 : 1 + ilog2c(n >> 1); }
// av1_get_tx_scale_tab (Codec/full_loop.h:53) as av1_get_tx_scale computes it: by the block's pixel count
__host__ __device__ constexpr int tx_log_scale(int s) { return tx_wide(s) * tx_high(s) > 1024 ? 2 : tx_wide(s) * tx_high(s) > 256 ? 1 : 0; }

} // namespace
#endif
