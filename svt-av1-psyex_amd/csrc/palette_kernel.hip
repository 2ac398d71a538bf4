// palette_kernel.hip -- the luma palette search, the palette rate of the candidates it keeps, and the palette prediction on gfx950:
// svt_hip_palette_search_batch and svt_hip_palette_pred_batch.
//
// Reference functions restated (Source/Lib/Codec):
//   search_palette_luma, palette_rd_y, optimize_palette_colors, av1_remove_duplicates, extend_palette_color_map   palette.c:64-76, :232-428
//   svt_av1_palette_color_cost_y, svt_av1_index_color_cache, delta_encode_cost                                   palette.c:78-143
//   svt_av1_cost_color_map, cost_and_tokenize_map (the rate side)                                                palette.c:487-547
//   svt_av1_k_means_dim1_c, svt_av1_calc_indices_dim1_c, calc_centroids, calc_total_dist, lcg_rand16             k_means_template.h, random.h
//   svt_av1_count_colors, svt_av1_count_colors_highbd                                                           pic_analysis_process.c:1809-1846
//   svt_aom_get_palette_color_index_context_optimized                                                           cabac_context_model.c:2453-2560
//   the palette branch of the luma rate, svt_aom_write_uniform_cost                                             rd_cost.c:679-706, entropy_coding.c:4206
//   the palette branch of svt_av1_predict_intra_block{,_16bit}                                                  enc_intra_prediction.c:501-510, :647-656
//
// Lay-out of the search: one wave per job, four jobs per workgroup, no workgroup barrier.
//   1  the histogram of the rows x cols samples in the wave's LDS (LDS atomics; the bin index is bounded before the access)
//   2  the live bins (at most 64, or the job ends) are compacted in ascending order to one (value, count) pair per lane; the bin then holds its
//      lane, and one more pass over the samples leaves each sample's lane in LDS, so no later step reads the source plane again -- but for the
//      one sample an empty k-means cluster takes
//   3  top_colors: eight wave maxima over count << 10 | (1023 - value)
//   4  k-means runs on the pairs: lane j holds centroid j, the assignment is per lane against the centroids read as scalars, a cluster's
//      count and sum and the 64-bit total distance are wave sums weighted by the lane's count -- the reference's integer sums exactly
//   5  a candidate: the cache snap per lane, rank among the distinct centroids by shuffles, the sorted unique palette in LDS; each lane
//      assigns its value an index, the map is that table applied to the samples' lanes with the extension folded into the addressing;
//      the map cost is a sum over the cropped positions in any order
// The prediction recomputes a sample's index from its value against the candidate's colours: at most eight comparisons, no histogram.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <type_traits>
#include "batch_host.h"
#include "../../include/svt_hip_palette.h"
#include "wave_ops.h"

namespace {

constexpr int kWaves   = 4;    // jobs per workgroup
constexpr int kSamples = 4096; // of a 64 x 64 block
constexpr int kMaxItr  = 50;
constexpr int kMaxN    = SVT_HIP_PALETTE_MAX_SIZE;

template <bool HBD> struct WaveLds {
    uint32_t hist[HBD ? 1024 : 256]; // counts, then the lane that holds the value
    uint32_t pairs[64];              // value | count << 16 of the live bins, ascending
    uint8_t  bin[kSamples];          // the lane of each sample of the cropped block, stride width
    uint8_t  map[kSamples];          // the candidate's colour map, width x height
    uint8_t  lane_index[64];         // the candidate's colour index of each lane's value
    int32_t  pal[kMaxN];             // the candidate's sorted unique centroids
    int32_t  out[kMaxN];             // out_cache_colors
    uint16_t cache[SVT_HIP_PALETTE_MAX_CACHE];
};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int log2_of(int v) { return 31 - __clz(v); }

// svt_av1_allow_palette: the block sizes from BLOCK_8X8 on in the enum without a side of 128
__device__ __forceinline__ bool size_allowed(int w, int h) {
    const int lo = w < h ? w : h, hi = w < h ? h : w;
    if (lo < 4 || hi > 64 || (w & (w - 1)) || (h & (h - 1)) || hi > 4 * lo) return false;
    return lo >= 8 || hi == 16;
}

// the checks both kernels make of a search job before anything of it is used as an address
__device__ __forceinline__ bool shape_ok(int w, int h, int rows, int cols, uint32_t src_offset, uint32_t src_stride, uint64_t src_samples) {
    if (!size_allowed(w, h) || rows == 0 || rows > h || cols == 0 || cols > w) return false;
    return (uint64_t)src_offset + (uint64_t)(rows - 1) * src_stride + (uint32_t)cols <= src_samples;
}

__device__ __forceinline__ int ceil_log2(int n) { return n < 2 ? 0 : 32 - __clz(n - 1); } // av1_ceil_log2

// delta_encode_cost with min_val = 1
__device__ __forceinline__ int delta_encode_cost(const int32_t *colors, int num, int bit_depth) {
    if (num <= 0) return 0;
    int bits_cost = bit_depth;
    if (num == 1) return bits_cost;
    bits_cost += 2;
    int max_delta = 0;
    for (int i = 1; i < num; ++i) {
        const int delta = colors[i] - colors[i - 1];
        if (delta > max_delta) max_delta = delta;
    }
    const int min_bits       = bit_depth - 3;
    int       bits_per_delta = ceil_log2(max_delta + 1 - 1);
    if (bits_per_delta < min_bits) bits_per_delta = min_bits;
    int range = (1 << bit_depth) - colors[0] - 1;
    for (int i = 0; i < num - 1; ++i) {
        bits_cost += bits_per_delta;
        range -= colors[i + 1] - colors[i];
        const int r = ceil_log2(range);
        if (r < bits_per_delta) bits_per_delta = r;
    }
    return bits_cost;
}

// svt_av1_palette_color_cost_y: every lane runs it on the same values (pal, cache and out are the wave's LDS)
__device__ __forceinline__ int color_cost_y(const int32_t *pal, int n, int max_val, const uint16_t *cache, int n_cache, int bit_depth, int32_t *out) {
    int n_out = 0;
    if (n_cache <= 0) {
        for (int i = 0; i < n; ++i) out[i] = pal[i] > max_val ? max_val : pal[i];
        n_out = n;
    } else {
        uint32_t in_cache = 0;
        int      n_in     = 0;
        for (int i = 0; i < n_cache && n_in < n; ++i)
            for (int j = 0; j < n; ++j)
                if ((pal[j] > max_val ? max_val : pal[j]) == (int)cache[i]) {
                    in_cache |= 1u << j;
                    ++n_in;
                    break;
                }
        for (int i = 0; i < n; ++i)
            if (!((in_cache >> i) & 1u)) out[n_out++] = pal[i] > max_val ? max_val : pal[i];
    }
    return (n_cache + delta_encode_cost(out, n_out, bit_depth)) * 512; // av1_cost_literal
}

__device__ __forceinline__ int write_uniform_cost(int n, int v) { // svt_aom_write_uniform_cost
    const int l = n > 0 ? 32 - __clz(n) : 0; // get_unsigned_bits
    const int m = (1 << l) - n;
    if (l == 0) return 0;
    return (v < m ? l - 1 : l) * 512;
}

// svt_aom_get_palette_color_index_context_optimized: the context, and the remapped index in *color_idx
__device__ __forceinline__ int color_index_context(const uint8_t *map, int stride, int r, int c, int *color_idx) {
    int n0 = c > 0 ? map[r * stride + c - 1] : -1;
    int n1 = r > 0 ? map[(r - 1) * stride + c] : -1;
    int n2 = (c > 0 && r > 0) ? map[(r - 1) * stride + c - 1] : -1;
    int s0 = 2, s1 = 2, s2 = 1;
    if (n0 == n1) {
        s0 += s1;
        n1 = -1;
        if (n0 == n2) {
            s0 += s2;
            n2 = -1;
        }
    } else if (n0 == n2) {
        s0 += s2;
        n2 = -1;
    } else if (n1 == n2) {
        s1 += s2;
        n2 = -1;
    }
    // The reference moves the valid neighbours to the front before it sorts; the three exchanges below are a sorting network on the score, and
    // an invalid neighbour with score 0 sinks to the end by itself.  Equal scores of valid neighbours only occur as (2, 2, 1), all three valid.
    int cr0 = n0, cr1 = n1, cr2 = n2, sr0 = n0 == -1 ? 0 : s0, sr1 = n1 == -1 ? 0 : s1, sr2 = n2 == -1 ? 0 : s2;
    int t;
    if (sr0 < sr1 || (sr0 == sr1 && cr0 > cr1)) { t = sr0; sr0 = sr1; sr1 = t; t = cr0; cr0 = cr1; cr1 = t; }
    if (sr0 < sr2) { t = sr0; sr0 = sr2; sr2 = t; t = cr0; cr0 = cr2; cr2 = t; }
    if (sr1 < sr2) { t = sr1; sr1 = sr2; sr2 = t; t = cr1; cr1 = cr2; cr2 = t; }
    const int cur  = map[r * stride + c];
    int       idx  = cur, same = -1;
    if (cr0 > cur) idx++; else if (cr0 == cur) same = 0;
    if (cr1 > cur) idx++; else if (cr1 == cur) same = 1;
    if (cr2 > cur) idx++; else if (cr2 == cur) same = 2;
    *color_idx = same != -1 ? same : idx;
    const int hash = sr0 + 2 * sr1 + 2 * sr2; // 1..8
    return hash == 2 ? 0 : 9 - hash; // svt_aom_palette_color_index_context_lookup {-, -, 0, -, -, 4, 3, 2, 1}
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void palette_search_kernel(const SvtHipPaletteDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    __shared__ WaveLds<HBD> lds[kWaves];
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    WaveLds<HBD>                 &L  = lds[wave];
    const SvtHipPaletteJob *const jp = d.jobs + job; // read field by field; the cache is read by the lanes themselves
    const uint32_t src_offset = jp->src_offset, map_offset = jp->map_offset;
    const int      w = jp->width, h = jp->height, rows = jp->rows, cols = jp->cols, n_cache = jp->n_cache, bsize_ctx = jp->bsize_ctx, mode_ctx = jp->mode_ctx;
    const int      max_val = HBD ? (1 << d.bit_depth) - 1 : 255;
    constexpr int  kBins   = HBD ? 1024 : 256;

    bool ok = shape_ok(w, h, rows, cols, src_offset, d.src_stride, d.src_samples) && n_cache <= SVT_HIP_PALETTE_MAX_CACHE &&
              bsize_ctx < SVT_HIP_PALETTE_BSIZE_CTXS && mode_ctx < SVT_HIP_PALETTE_MODE_CTXS;
    const int cached = ok && lane < n_cache ? jp->color_cache[lane] : 0; // may lie above max_val: an 8-bit search of a 10-bit encode
    if (ok && d.color_maps) ok = (uint64_t)map_offset + (uint64_t)SVT_HIP_PALETTE_MAX_CANDS * (uint32_t)(w * h) <= d.map_bytes;
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_PALETTE_UNDEFINED;
        return;
    }
    const Px *const src = (const Px *)d.src + src_offset;
    const int       n   = rows * cols; // of `data`
    SvtHipPaletteResult *const res = d.results + job;

    // 1: the histogram
    for (int i = lane; i < kBins; i += 64) L.hist[i] = 0;
    if (lane < SVT_HIP_PALETTE_MAX_CACHE) L.cache[lane] = (uint16_t)cached;
    wave_sync();
    bool bad = false;
    for (int i = lane; i < n; i += 64) {
        const int      r = i / cols, c = i - r * cols;
        const uint32_t v = src[(size_t)r * d.src_stride + c];
        if (v < (uint32_t)kBins && (int)v <= max_val) atomicAdd(&L.hist[v], 1u); // never a bin outside the wave's slice
        else bad = true;
    }
    wave_sync();
    if (__ballot(bad)) { // svt_av1_count_colors_highbd returns 0
        if (lane == 0) { res->n_colors = 0; res->n_cands = 0; d.status[job] = SVT_HIP_PALETTE_OK; }
        return;
    }

    // 2: one (value, count) per lane, ascending
    int colors = 0;
    for (int k = 0; k < kBins / 64; k++) {
        const int      b    = k * 64 + lane;
        const uint32_t c    = L.hist[b];
        const uint64_t live = __ballot(c != 0);
        const int      pos  = colors + __popcll(live & ((1ull << lane) - 1ull));
        if (c != 0 && pos < 64) {
            L.pairs[pos] = (uint32_t)b | (c << 16);
            L.hist[b]    = (uint32_t)pos;
        }
        colors += __popcll(live);
    }
    colors = uniform(colors);
    if (!(colors > 1 && colors <= 64)) {
        if (lane == 0) { res->n_colors = (uint32_t)colors; res->n_cands = 0; d.status[job] = SVT_HIP_PALETTE_OK; }
        return;
    }
    wave_sync();
    const bool     live = lane < colors;
    const int      val  = live ? (int)(L.pairs[lane] & 0xFFFFu) : 0;
    const uint32_t cnt  = live ? L.pairs[lane] >> 16 : 0u;
    for (int i = lane; i < n; i += 64) {
        const int r = i / cols, c = i - r * cols;
        L.bin[r * w + c] = (uint8_t)L.hist[src[(size_t)r * d.src_stride + c] & (kBins - 1)]; // bounded again: the plane is read a second time
    }
    wave_sync();
    const int      lb = __builtin_amdgcn_readlane(val, 0), ub = __builtin_amdgcn_readlane(val, colors - 1);
    const uint32_t data0 = src[0];
    const int      top_n = colors < kMaxN ? colors : kMaxN;

    // 3: top_colors, lane i its i-th
    int top = 0;
    {
        uint32_t work = cnt;
        for (int i = 0; i < top_n; i++) {
            const uint32_t best = wave_max<uint32_t>(work ? (work << 10) | (uint32_t)(1023 - val) : 0u); // the lower value among equal counts
            const int      tv   = 1023 - (int)(best & 1023u);
            if (lane == i) top = tv;
            if (live && val == tv) work = 0;
        }
    }

    const int32_t *const map_tab  = d.palette_ycolor_fac_bitss;
    const int            mode_bits = d.palette_ymode_fac_bits[(bsize_ctx * SVT_HIP_PALETTE_MODE_CTXS + mode_ctx) * 3 + 1];
    int                  n_cands  = 0;
    const int            lw       = log2_of(w);

    // 5: palette_rd_y and the rate of the candidate whose centroid i is lane i's `cen`, i < nc
    auto candidate = [&](int cen, int nc) __attribute__((always_inline)) {
        const bool in = lane < nc;
        if (n_cache > 0 && in) { // optimize_palette_colors
            int min_diff = abs(cen - (int)L.cache[0]), idx = 0;
            for (int q = 1; q < n_cache; ++q) {
                const int diff = abs(cen - (int)L.cache[q]);
                if (diff < min_diff) { min_diff = diff; idx = q; }
            }
            if (min_diff <= 1) cen = L.cache[idx];
        }
        bool first = in; // of its value among the centroids
#pragma unroll
        for (int q = 0; q < kMaxN; q++) {
            const int cq = __builtin_amdgcn_readlane(cen, q);
            if (q < nc && q < lane && cq == cen) first = false;
        }
        const uint64_t firsts = __ballot(first);
        const int      k      = __popcll(firsts);
        if (k <= 2) return; // palette_size_array[] > 2 or the candidate is not counted
        int below = 0;
#pragma unroll
        for (int q = 0; q < kMaxN; q++) {
            const int cq = __builtin_amdgcn_readlane(cen, q);
            if (((firsts >> q) & 1ull) && cq < cen) below++;
        }
        wave_sync(); // the last candidate's readers are done
        if (first) L.pal[below] = cen;
        wave_sync();
        { // svt_av1_calc_indices_dim1_c for the lane's value
            int min_dist = (val - L.pal[0]) * (val - L.pal[0]), idx = 0;
            for (int q = 1; q < k; ++q) {
                const int dist = (val - L.pal[q]) * (val - L.pal[q]);
                if (dist < min_dist) { min_dist = dist; idx = q; }
            }
            L.lane_index[lane] = (uint8_t)idx;
        }
        wave_sync();
        uint8_t *const gmap = d.color_maps ? d.color_maps + map_offset + (size_t)n_cands * (uint32_t)(w * h) : nullptr;
        for (int p = lane * 4; p < w * h; p += 256) { // four positions of one row; extend_palette_color_map is the clamp
            const int r = p >> lw, c = p & (w - 1), rr = (r < rows ? r : rows - 1) * w;
            uint32_t  m = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) m |= (uint32_t)L.lane_index[L.bin[rr + (c + q < cols ? c + q : cols - 1)]] << (8 * q);
            *(uint32_t *)(L.map + p) = m;
            if (gmap) {
                if ((((uintptr_t)gmap) & 3u) == 0) *(uint32_t *)(gmap + p) = m;
                else { gmap[p] = (uint8_t)m; gmap[p + 1] = (uint8_t)(m >> 8); gmap[p + 2] = (uint8_t)(m >> 16); gmap[p + 3] = (uint8_t)(m >> 24); }
            }
        }
        wave_sync();
        uint32_t map_cost = 0;
        if (!d.reduce_palette_cost_precision) { // cost_and_tokenize_map: every position of the cropped block but the first
            const int32_t *const tab = map_tab + (k - 2) * 40;
            uint32_t             sum = 0;
            for (int i = lane; i < n; i += 64) {
                if (i == 0) continue;
                const int r = i / cols, c = i - r * cols;
                int       idx;
                const int ctx = color_index_context(L.map, w, r, c, &idx);
                sum += (uint32_t)tab[ctx * 8 + idx];
            }
            map_cost = wave_sum_dpp(sum);
        }
        const int first_index = L.map[0];
        const int color_cost  = color_cost_y(L.pal, k, max_val, L.cache, n_cache, d.cost_bit_depth, L.out);
        if (lane == 0) {
            SvtHipPaletteCand *const rec = res->cands + n_cands; // field by field: a record built on the stack would live in scratch
            const int index0_cost = write_uniform_cost(k, first_index), size_cost = d.palette_ysize_fac_bits[bsize_ctx * 8 + k - 2];
            rec->size        = (uint8_t)k;
            rec->first_index = (uint8_t)first_index;
#pragma unroll
            for (int q = 0; q < kMaxN; q++) rec->colors[q] = q < k ? (uint16_t)(L.pal[q] > max_val ? max_val : L.pal[q] < 0 ? 0 : L.pal[q]) : (uint16_t)0;
            rec->top_over    = (uint8_t)(L.pal[k - 1] > max_val); // the indices were computed against max_val + 1
            rec->reserved    = 0;
            rec->color_cost  = color_cost;
            rec->map_cost    = (int32_t)map_cost;
            rec->index0_cost = index0_cost;
            rec->size_cost   = size_cost;
            rec->rate        = mode_bits + size_cost + index0_cost + color_cost + (int32_t)map_cost;
        }
        n_cands++;
    };

    // the dominant colours directly
    for (int nc = top_n; nc >= 2; nc -= d.dominant_color_step) candidate(top, nc);

    // 4: k-means
    for (int nc = top_n; nc >= 2; --nc) {
        int cen;
        if (colors == 2) cen = lane == 0 ? lb : ub;
        else {
            cen = lb + (2 * lane + 1) * (ub - lb) / nc / 2;
            int      index;
            uint64_t this_dist;
            auto     assign = [&]() __attribute__((always_inline)) { // calc_indices and calc_total_dist
                int min_dist = (val - __builtin_amdgcn_readlane(cen, 0)) * (val - __builtin_amdgcn_readlane(cen, 0));
                index        = 0;
#pragma unroll
                for (int q = 1; q < kMaxN; q++) {
                    const int cq = __builtin_amdgcn_readlane(cen, q), dist = (val - cq) * (val - cq);
                    if (q < nc && dist < min_dist) { min_dist = dist; index = q; }
                }
                this_dist = wave_sum64_dpp(live ? (uint64_t)(uint32_t)min_dist * cnt : 0ull);
            };
            assign();
            for (int it = 0; it < kMaxItr; ++it) {
                const uint64_t pre_dist = this_dist;
                const int      pre_cen  = cen;
                uint32_t       state    = data0; // calc_centroids
                for (int q = 0; q < nc; q++) {
                    const bool     mine  = live && index == q;
                    const uint32_t count = wave_sum_dpp(mine ? cnt : 0u), sum = wave_sum_dpp(mine ? cnt * (uint32_t)val : 0u);
                    int            next;
                    if (count == 0) { // an empty cluster: data[lcg_rand16(&state) % n]
                        state = state * 1103515245u + 12345u;
                        const int at = (int)(((state / 65536u) % 32768u) % (uint32_t)n), r = at / cols;
                        next = src[(size_t)r * d.src_stride + (at - r * cols)];
                    } else next = (int)((sum + (count >> 1)) / count); // DIVIDE_AND_ROUND
                    if (lane == q) cen = next;
                }
                assign();
                if (this_dist > pre_dist) { // cannot happen for one dimension; the reference's restore all the same
                    cen = pre_cen;
                    break;
                }
                if (!__ballot(lane < nc && cen != pre_cen)) break;
            }
        }
        candidate(cen, nc);
    }
    if (lane == 0) { res->n_colors = (uint32_t)colors; res->n_cands = (uint32_t)n_cands; d.status[job] = SVT_HIP_PALETTE_OK; }
}

template <bool HBD> __global__ __launch_bounds__(64 * kWaves) void palette_pred_kernel(const SvtHipPalettePredDesc d) {
    using Px = typename std::conditional<HBD, uint16_t, uint8_t>::type;
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job  = blockIdx.x * (uint32_t)kWaves + (uint32_t)wave;
    if (job >= d.n_jobs) return;
    const SvtHipPalettePredJob p = d.jobs[job];
    bool                       ok = p.search_index < d.n_search_jobs && d.search_status[p.search_index] == SVT_HIP_PALETTE_OK;
    SvtHipPaletteJob           j;
    SvtHipPaletteCand          cand;
    memset(&j, 0, sizeof(j));
    memset(&cand, 0, sizeof(cand));
    if (ok) {
        j  = d.search_jobs[p.search_index];
        ok = shape_ok(j.width, j.height, j.rows, j.cols, j.src_offset, d.src_stride, d.src_samples) && p.cand_index < d.search_results[p.search_index].n_cands && p.cand_index < SVT_HIP_PALETTE_MAX_CANDS;
    }
    const int w = j.width, h = j.height, rows = j.rows, cols = j.cols;
    if (ok) {
        cand = d.search_results[p.search_index].cands[p.cand_index];
        ok   = cand.size >= 3 && cand.size <= kMaxN && (uint64_t)p.dst_offset + (uint64_t)(h - 1) * d.dst_stride + (uint32_t)w <= d.dst_samples &&
             (!d.color_map || (uint64_t)p.map_offset + (uint32_t)(w * h) <= d.map_bytes);
    }
    if (!ok) {
        if (lane == 0) d.status[job] = SVT_HIP_PALETTE_UNDEFINED;
        return;
    }
    const Px *const src  = (const Px *)d.src + j.src_offset;
    Px *const       dst  = (Px *)d.dst + p.dst_offset;
    uint8_t *const  gmap = d.color_map ? d.color_map + p.map_offset : nullptr;
    const int       lw = log2_of(w), k = cand.size;
    const uint32_t  max_val = HBD ? 0xFFFFu : 0xFFu; // the reference's clamp
    int             cen[kMaxN]; // what palette_rd_y computed the indices against: the colours, the last one before its clip
#pragma unroll
    for (int s = 0; s < kMaxN; s++) cen[s] = (int)cand.colors[s] + (s == k - 1 && cand.top_over ? 1 : 0);
    for (int at = lane * 4; at < w * h; at += 256) {
        const int r = at >> lw, c = at & (w - 1);
        const Px *row = src + (size_t)(r < rows ? r : rows - 1) * d.src_stride;
        uint32_t  m = 0, o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int v        = row[c + q < cols ? c + q : cols - 1];
            int       min_dist = (v - cen[0]) * (v - cen[0]), idx = 0;
            uint32_t  color    = cand.colors[0];
#pragma unroll
            for (int s = 1; s < kMaxN; s++) {
                const int dist = (v - cen[s]) * (v - cen[s]);
                if (s < k && dist < min_dist) { min_dist = dist; idx = s; color = cand.colors[s]; }
            }
            m |= (uint32_t)idx << (8 * q);
            o[q] = color > max_val ? max_val : color;
        }
        Px *const t = dst + (size_t)r * d.dst_stride + c;
        if (HBD) {
            if (((uintptr_t)t & 7u) == 0) *(uint2 *)t = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
            else { t[0] = (Px)o[0]; t[1] = (Px)o[1]; t[2] = (Px)o[2]; t[3] = (Px)o[3]; }
        } else {
            if (((uintptr_t)t & 3u) == 0) *(uint32_t *)t = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            else { t[0] = (Px)o[0]; t[1] = (Px)o[1]; t[2] = (Px)o[2]; t[3] = (Px)o[3]; }
        }
        if (gmap) {
            if ((((uintptr_t)gmap) & 3u) == 0) *(uint32_t *)(gmap + at) = m;
            else { gmap[at] = (uint8_t)m; gmap[at + 1] = (uint8_t)(m >> 8); gmap[at + 2] = (uint8_t)(m >> 16); gmap[at + 3] = (uint8_t)(m >> 24); }
        }
    }
    if (lane == 0) d.status[job] = SVT_HIP_PALETTE_OK;
}

} // namespace

extern "C" {

int svt_hip_palette_check_desc(const SvtHipPaletteDesc *d) {
    if (!d) BAD("svt_hip_palette_check_desc: null descriptor");
    if (!d->src || !d->jobs || !d->results || !d->status || !d->palette_ycolor_fac_bitss || !d->palette_ysize_fac_bits || !d->palette_ymode_fac_bits)
        BAD("svt_hip_palette_check_desc: a mandatory pointer (src, jobs, results, status, palette_ycolor_fac_bitss, palette_ysize_fac_bits, palette_ymode_fac_bits) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_palette_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->cost_bit_depth != 8 && d->cost_bit_depth != 10) BAD("svt_hip_palette_check_desc: cost_bit_depth %u (8 or 10)", d->cost_bit_depth);
    if (d->bit_depth == 10 && d->cost_bit_depth != 10)
        BAD("svt_hip_palette_check_desc: bit_depth 10 with cost_bit_depth %u (10-bit planes are searched in a 10-bit encode only)", d->cost_bit_depth);
    if (d->dominant_color_step != 1 && d->dominant_color_step != 2) BAD("svt_hip_palette_check_desc: dominant_color_step %u (1 or 2)", d->dominant_color_step);
    if (d->src_stride == 0 || d->src_samples == 0)
        BAD("svt_hip_palette_check_desc: src_stride %u / src_samples %llu is zero", d->src_stride, (unsigned long long)d->src_samples);
    if (d->color_maps && d->map_bytes == 0) BAD("svt_hip_palette_check_desc: color_maps with map_bytes zero");
    return SVT_HIP_OK;
}

int svt_hip_palette_pred_check_desc(const SvtHipPalettePredDesc *d) {
    if (!d) BAD("svt_hip_palette_pred_check_desc: null descriptor");
    if (!d->src || !d->dst || !d->search_jobs || !d->search_results || !d->search_status || !d->jobs || !d->status)
        BAD("svt_hip_palette_pred_check_desc: a mandatory pointer (src, dst, search_jobs, search_results, search_status, jobs, status) is null");
    if (d->bit_depth != 8 && d->bit_depth != 10) BAD("svt_hip_palette_pred_check_desc: bit_depth %u (8 or 10)", d->bit_depth);
    if (d->src_stride == 0 || d->src_samples == 0 || d->dst_stride == 0 || d->dst_samples == 0)
        BAD("svt_hip_palette_pred_check_desc: a stride or sample count is zero (src %u / %llu, dst %u / %llu)", d->src_stride, (unsigned long long)d->src_samples,
            d->dst_stride, (unsigned long long)d->dst_samples);
    if (d->n_search_jobs == 0) BAD("svt_hip_palette_pred_check_desc: n_search_jobs is zero");
    if (d->color_map && d->map_bytes == 0) BAD("svt_hip_palette_pred_check_desc: color_map with map_bytes zero");
    return SVT_HIP_OK;
}

size_t svt_hip_palette_layout(int what, int field) {
#define D(f) offsetof(SvtHipPaletteDesc, f)
#define J(f) offsetof(SvtHipPaletteJob, f)
#define C(f) offsetof(SvtHipPaletteCand, f)
#define R(f) offsetof(SvtHipPaletteResult, f)
#define P(f) offsetof(SvtHipPalettePredJob, f)
#define Q(f) offsetof(SvtHipPalettePredDesc, f)
    static const size_t desc[] = {D(bit_depth), D(cost_bit_depth), D(dominant_color_step), D(reduce_palette_cost_precision), D(n_jobs), D(src), D(src_stride),
                                  D(reserved), D(src_samples), D(palette_ycolor_fac_bitss), D(palette_ysize_fac_bits), D(palette_ymode_fac_bits), D(jobs),
                                  D(results), D(status), D(color_maps), D(map_bytes)};
    static const size_t job[]  = {J(src_offset), J(map_offset), J(width), J(height), J(rows), J(cols), J(n_cache), J(bsize_ctx), J(mode_ctx), J(reserved),
                                  J(color_cache)};
    static const size_t cand[] = {C(size), C(first_index), C(colors), C(top_over), C(reserved), C(color_cost), C(map_cost), C(index0_cost), C(size_cost), C(rate)};
    static const size_t res[]  = {R(n_colors), R(n_cands), R(cands)};
    static const size_t pjob[] = {P(search_index), P(cand_index), P(dst_offset), P(map_offset)};
    static const size_t pdes[] = {Q(bit_depth), Q(reserved), Q(n_jobs), Q(n_search_jobs), Q(src_stride), Q(src), Q(src_samples), Q(dst), Q(dst_stride),
                                  Q(reserved2), Q(dst_samples), Q(search_jobs), Q(search_results), Q(search_status), Q(jobs), Q(status), Q(color_map),
                                  Q(map_bytes)};
#undef D
#undef J
#undef C
#undef R
#undef P
#undef Q
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipPaletteDesc>(desc),  layout_row<SvtHipPaletteJob>(job),     layout_row<SvtHipPaletteCand>(cand),
                                    layout_row<SvtHipPaletteResult>(res), layout_row<SvtHipPalettePredJob>(pjob), layout_row<SvtHipPalettePredDesc>(pdes)};
    return layout_lookup(rows, what, field);
}

int svt_hip_palette_search_batch(SvtHipContext *ctx, const SvtHipPaletteDesc *d) {
    return enqueue_batch("svt_hip_palette_search_batch", ctx, d, svt_hip_palette_check_desc, &SvtHipPaletteDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, palette_search_kernel<true>, palette_search_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

int svt_hip_palette_pred_batch(SvtHipContext *ctx, const SvtHipPalettePredDesc *d) {
    return enqueue_batch("svt_hip_palette_pred_batch", ctx, d, svt_hip_palette_pred_check_desc, &SvtHipPalettePredDesc::n_jobs, [=] {
        hipLaunchKernelGGL(pick_hbd(d->bit_depth, palette_pred_kernel<true>, palette_pred_kernel<false>), dim3(ceil_div(d->n_jobs, kWaves)), dim3(64 * kWaves), 0,
                           ctx->stream, *d);
    });
}

} // extern "C"
