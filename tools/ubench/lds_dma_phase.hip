// lds_dma_phase.hip -- does the direct-to-LDS load (global_load_lds_dwordx4, csrc/lds_dma.h) honour source addresses of any byte alignment,
// as the plain unaligned 16-byte global loads of the ME window staging do?  One wave copies a 2-D window (6 vectors per row x 75 rows: 450
// vectors, so eight instructions, the last one partial) from a seeded byte buffer into LDS through lds_dma_window() and back out, for every
// source byte phase 0..15 and row strides = 0, 4, 8, 12 (mod 16), and a linear copy of 70 vectors through lds_dma_copy() for every phase.
// A last column copies rows of four pieces to a pitch of five through lds_dma_load16() with every fifth lane switched off in the MIDDLE of an
// instruction -- the source views of me_kernel.hip -- and checks that the holes keep their sentinel.
// Each copy is compared with the same bytes read by plain byte loads (and with the host's copy of the buffer); the LDS bytes around the
// destination must keep their sentinel.  Prints a phase x stride table of right / wrong; exit status 1 on any wrong byte.  Reads stay inside
// the buffer.
// Build: hipcc --offload-arch=gfx950 -O3 lds_dma_phase.hip -o lds_dma_phase ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../svt-av1-psyex_amd/csrc/lds_dma.h"

constexpr int kVpr = 6, kRows = 75, kVec = kVpr * kRows, kLinear = 70; // window: 96 bytes a row
constexpr int kGuard = 64, kDst = kGuard, kLdsBytes = kGuard + kVec * 16 + kGuard;
constexpr int kBase = 64; // byte offset of phase 0 in the buffer
constexpr uint8_t kSentinel = 0xA5;

extern __shared__ __attribute__((aligned(16))) uint8_t g_lds[];

// linear == 1: `rows` is the vector count of a linear copy.  linear == 2: the holed view copy (piece n = row n / 5, part n % 5, part 4 skipped).  via_lds: what came through LDS (guards included); plain: the same bytes by byte loads
__global__ void __launch_bounds__(64) copy_window(const uint8_t *src, uint32_t stride, int vpr, int rows, int linear, uint8_t *via_lds, uint8_t *plain) {
    const int lane = threadIdx.x, nvec = linear == 1 ? rows : linear == 2 ? rows * 5 : vpr * rows;
    for (int i = lane; i < kLdsBytes / 4; i += 64) reinterpret_cast<uint32_t *>(g_lds)[i] = 0x01010101u * kSentinel;
    lds_dma_after_stores();
    if (linear == 2) {
        for (int b0 = 0; b0 < nvec; b0 += 64) { // uniform
            const int n = b0 + lane, row = n / 5, cc = n - row * 5;
            if (n < nvec && cc < 4) lds_dma_load16(src + (size_t)row * stride + cc * 16, g_lds, kDst + (uint32_t)b0 * 16);
        }
    } else if (linear) lds_dma_copy(src, g_lds, kDst, nvec);
    else lds_dma_window(src, stride, vpr, rows, g_lds, kDst);
    lds_dma_wait();
    for (int i = lane; i < kLdsBytes / 4; i += 64) reinterpret_cast<uint32_t *>(via_lds)[i] = reinterpret_cast<const uint32_t *>(g_lds)[i];
    for (int i = lane; i < nvec * 16; i += 64) {
        const int per = linear == 2 ? 5 : vpr, k = i >> 4, row = linear == 1 ? 0 : k / per, c = linear == 1 ? k : k - row * per;
        plain[i] = (linear == 2 && c == 4) ? kSentinel : src[(size_t)row * stride + c * 16 + (i & 15)];
    }
}

#define CHECK(call)                                                                                  \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) { printf("%s: %s\n", #call, hipGetErrorString(e_)); return 2; }        \
    } while (0)

int main() {
    const uint32_t strides[4] = {3968, 3972, 3976, 3980}; // = 0, 4, 8, 12 (mod 16); 3976 is the bench's plane stride
    const size_t   buf_bytes  = kBase + 16 + (size_t)kRows * strides[3] + 128;
    std::vector<uint8_t> host(buf_bytes);
    uint32_t s = 0x2545F491u;
    for (size_t i = 0; i < buf_bytes; i++) { s = s * 1664525u + 1013904223u; host[i] = (uint8_t)(s >> 24); }
    uint8_t *buf, *via_lds, *plain;
    CHECK(hipMalloc(&buf, buf_bytes));
    CHECK(hipMalloc(&via_lds, kLdsBytes));
    CHECK(hipMalloc(&plain, kVec * 16));
    CHECK(hipMemcpy(buf, host.data(), buf_bytes, hipMemcpyHostToDevice));
    std::vector<uint8_t> got(kLdsBytes), ref(kVec * 16);
    int wrong_total = 0;
    printf("global_load_lds_dwordx4: window %d vectors x %d rows, and a linear copy of %d vectors; wrong bytes (0 = right)\n", kVpr, kRows, kLinear);
    printf("phase  stride%%16=0  stride%%16=4  stride%%16=8  stride%%16=12       linear   holed view\n");
    for (int phase = 0; phase < 16; phase++) {
        printf("%5d", phase);
        for (int col = 0; col < 6; col++) {
            const int      linear = col == 4 ? 1 : col == 5 ? 2 : 0;
            const uint32_t stride = linear == 1 ? 0 : linear == 2 ? strides[2] : strides[col];
            const int      nvec   = linear == 1 ? kLinear : linear == 2 ? kRows * 5 : kVec;
            CHECK(hipMemset(via_lds, 0, kLdsBytes));
            CHECK(hipMemset(plain, 0, kVec * 16));
            copy_window<<<1, 64, kLdsBytes>>>(buf + kBase + phase, stride, kVpr, linear == 1 ? kLinear : kRows, linear, via_lds, plain);
            CHECK(hipGetLastError());
            CHECK(hipDeviceSynchronize());
            CHECK(hipMemcpy(got.data(), via_lds, kLdsBytes, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(ref.data(), plain, kVec * 16, hipMemcpyDeviceToHost));
            int wrong = 0;
            for (int i = 0; i < kLdsBytes; i++) {
                const int j = i - kDst;
                if (j < 0 || j >= nvec * 16) { wrong += got[i] != kSentinel; continue; } // around the destination: untouched
                const int per = linear == 2 ? 5 : kVpr, k = j >> 4, row = linear == 1 ? 0 : k / per, c = linear == 1 ? k : k - row * per;
                const uint8_t want = (linear == 2 && c == 4) ? kSentinel : host[kBase + phase + (size_t)row * stride + c * 16 + (j & 15)]; // a hole: untouched
                wrong += got[i] != ref[j] || ref[j] != want;
            }
            printf("  %11d", wrong);
            wrong_total += wrong;
        }
        printf("\n");
    }
    printf("%s\n", wrong_total ? "WRONG: some alignment class is not honoured" : "all right: every source byte phase and row stride copies exactly");
    return wrong_total ? 1 : 0;
}
