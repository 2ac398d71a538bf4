// gm_kernel.hip -- the device side of global-motion estimation on gfx950: svt_hip_gm_refine_batch, the refinement of the integerized models, and
// svt_hip_gm_correspondence_batch, the correspondences and picture sums taken from the ME results where the ME launch left them.
//
// Reference functions restated (Source/Lib/Codec):
//   svt_av1_refine_integerized_param, add_param_offset, force_wmtype, get_wmtype, svt_av1_is_enough_erroradvantage   global_motion.c:27-206
//   svt_av1_warp_error, warp_error                                                                                  enc_warped_motion.c:22-98
//   svt_get_shear_params, svt_warp_plane (the ROTZOOM rewrite), svt_av1_warp_affine_c                                warped_motion.c:569-712, :898-921
//   compute_global_motion (the picture SAD and its zero exit), the sums of svt_aom_global_motion_estimation         global_me.c:162-169, :354-360
//   correspondence_from_mvs                                                                                         global_motion.c:236-337
//
// The refinement is a chain of launches on the context stream.  gm_sad_kernel sums |reference - source| per reference.  gm_decide_kernel, one lane
// per job, holds everything sequential: it validates the job, applies the decisions of the evaluations of the launch before it in the reference's
// order (left, then right, each on a strict <), carries the whole EbWarpedMotionParams -- wmmat[4] and wmmat[5] of a ROTZOOM model as the last
// candidate that reached the warp left them -- and writes the next candidates with their shear parameters, or the job's outputs.  gm_eval_kernel
// is the hot one: a workgroup of four waves per (32x32 block, side, job), a wave per 8x8 tile at a time through warp_tile of warp_core.h, the SAD
// against the source over the tile's samples inside the picture, a wave reduction, an LDS reduction and one 64-bit integer atomic per workgroup.
// Nothing waits inside a kernel: a round sees its predecessor's sums because the stream orders the launches.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "batch_host.h"
#include "../../include/svt_hip_gm.h"
#include "wave_ops.h"
#include "warp_core.h"

namespace {

constexpr int kWaves = 4;
constexpr int kSlots = SVT_HIP_GM_ROUND_ERRORS;
constexpr int kSadRows = 16; // picture rows per workgroup of gm_sad_kernel

// What a job carries from launch to launch (in SvtHipGmRefineDesc.work, behind the sums)
struct GmState {
    int64_t  best_error;
    int32_t  mat[6];          // wm->wmmat as the reference holds it between two evaluations
    int32_t  cand_mat[2][6];  // per side: the matrix the samples are warped with
    int32_t  cand_shear[2][4];
    int32_t  cur, val[2];     // the round's parameter before it, and its left and right candidate
    uint8_t  run[2];          // per side: the candidate reaches the warp (else its error is 1, or the side does not exist)
    uint8_t  done, reserved;
    uint32_t pic_sad;
};

// work: uint32 sad[16] (8 used) | uint64 sums[n_jobs][kSlots] | GmState[n_jobs]
struct Work {
    uint32_t           *sad;
    unsigned long long *sums;
    GmState            *state;
};
__host__ __device__ inline Work work_of(void *p, uint32_t n_jobs) {
    Work w;
    w.sad   = (uint32_t *)p;
    w.sums  = (unsigned long long *)((char *)p + 64);
    w.state = (GmState *)((char *)p + 64 + (size_t)n_jobs * kSlots * 8);
    return w;
}
inline size_t work_bytes(uint32_t n_jobs) { return 64 + (size_t)n_jobs * (kSlots * 8 + sizeof(GmState)); }

__device__ __forceinline__ const uint8_t *origin_of(const SvtHipWarpRef &r) { return (const uint8_t *)r.plane + (size_t)r.org_y * r.stride + r.org_x; }

// ---- svt_nxm_sad_kernel of every reference picture against the source, mod 2^32 ----
__global__ __launch_bounds__(64 * kWaves) void gm_sad_kernel(const SvtHipGmRefineDesc d) {
    __shared__ uint32_t s_part[kWaves];
    const int      ref = (int)blockIdx.y, pw = d.src.width, ph = d.src.height;
    const uint8_t *a = origin_of(d.refs[ref]), *b = origin_of(d.src);
    const uint32_t sa = d.refs[ref].stride, sb = d.src.stride;
    const int      y0 = (int)blockIdx.x * kSadRows, y1 = y0 + kSadRows < ph ? y0 + kSadRows : ph;
    uint32_t       acc = 0;
    for (int y = y0; y < y1; y++)
        for (int x = (int)threadIdx.x; x < pw; x += 64 * kWaves) acc += (uint32_t)iabs((int)a[(size_t)y * sa + x] - (int)b[(size_t)y * sb + x]);
    acc = wave_sum_dpp(acc);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) t += s_part[w];
        atomicAdd(work_of(d.work, d.n_jobs).sad + ref, t);
    }
}

// ---- the decisions ----
__device__ __forceinline__ int neg32(int v) { return (int)(0u - (uint32_t)v); }

__device__ __forceinline__ void force_wmtype(int32_t *m, int type) { // IDENTITY never comes here
    if (type <= SVT_HIP_GM_TRANSLATION) { m[2] = 1 << 16; m[3] = 0; }
    if (type <= SVT_HIP_WARP_ROTZOOM) { m[4] = neg32(m[3]); m[5] = m[2]; }
}
__device__ __forceinline__ int get_wmtype(const int32_t *m) {
    if (m[5] == (1 << 16) && !m[4] && m[2] == (1 << 16) && !m[3]) return (!m[1] && !m[0]) ? 0 : SVT_HIP_GM_TRANSLATION;
    return (m[2] == m[5] && m[3] == neg32(m[4])) ? SVT_HIP_WARP_ROTZOOM : SVT_HIP_WARP_AFFINE;
}
// add_param_offset: GM_TRANS_PREC_DIFF 10 and GM_TRANS_MAX 1 << 12 for the translation, GM_ALPHA_PREC_DIFF 1 and GM_ALPHA_MAX 1 << 12 for the rest
__device__ __forceinline__ int add_param_offset(int p, int v, int offset) {
    const int scale = p < 2 ? 10 : 1, centre = (p == 2 || p == 5) ? 1 << 16 : 0;
    v = (int)((uint32_t)v - (uint32_t)centre) >> scale;
    v = clampi((int)((uint32_t)v + (uint32_t)offset), -(1 << 12), 1 << 12);
    return v * (1 << scale) + centre;
}
// svt_get_shear_params on the matrix as it stands: (1 or 0, the four parameters -- 0 when wmmat[2] <= 0)
__device__ __forceinline__ bool shear_of(const int32_t *m, int32_t *sh) {
    sh[0] = sh[1] = sh[2] = sh[3] = 0;
    if (m[2] <= 0) return false;
    return shear_params(m[2], m[3], m[4], m[5], &sh[0], &sh[1], &sh[2], &sh[3]);
}
// The head of svt_av1_warp_error for the matrix in st->mat: the shear test on it as it stands, then svt_warp_plane's rewrite if it is reached
__device__ __forceinline__ void set_candidate(GmState *st, int side, int type) {
    const bool ok = shear_of(st->mat, st->cand_shear[side]);
    st->run[side] = ok ? 1 : 0;
    if (!ok) return;
    if (type == SVT_HIP_WARP_ROTZOOM) { st->mat[5] = st->mat[2]; st->mat[4] = neg32(st->mat[3]); }
#pragma unroll
    for (int i = 0; i < 6; i++) st->cand_mat[side][i] = st->mat[i];
}
__device__ __forceinline__ void write_outputs(const SvtHipGmRefineDesc &d, uint32_t job, GmState *st, int wmtype, int status) {
    SvtHipWarpModel out;
    memset(&out, 0, sizeof(out));
    int32_t sh[4];
    out.valid = shear_of(st->mat, sh) ? 1 : 0;
#pragma unroll
    for (int i = 0; i < 6; i++) out.wmmat[i] = st->mat[i];
    out.alpha = (int16_t)sh[0]; out.beta = (int16_t)sh[1]; out.gamma = (int16_t)sh[2]; out.delta = (int16_t)sh[3];
    out.wmtype = (uint8_t)wmtype;
    d.models[job]     = out;
    d.best_error[job] = st->best_error;
    d.status[job]     = (uint8_t)status;
    st->run[0] = st->run[1] = 0;
    st->done   = 1;
}

// launch: 0 before the first evaluation; L >= 1 behind evaluation launch L - 1 and before launch L, which holds the jobs' round L - 1
__global__ __launch_bounds__(64) void gm_decide_kernel(const SvtHipGmRefineDesc d, const int launch) {
    const uint32_t job = blockIdx.x * 64u + threadIdx.x;
    if (job >= d.n_jobs) return;
    const Work               w  = work_of(d.work, d.n_jobs);
    GmState                 *st = w.state + job;
    const SvtHipGmRefineJob *jp = d.jobs + job;
    const int                type = jp->wmtype, n_params = 2 * type;
    const int64_t            mul = d.chess_refn ? 2 : 1;
    int64_t *const           errs = d.round_error ? d.round_error + (size_t)job * kSlots : nullptr;
    if (launch == 0) {
        if (jp->ref >= d.n_refs || type < SVT_HIP_GM_TRANSLATION || type > SVT_HIP_WARP_AFFINE) {
            d.status[job] = SVT_HIP_GM_UNDEFINED;
            st->done      = 1; // run[] is zero already: the entry cleared the work buffer
            return;
        }
        st->pic_sad    = w.sad[jp->ref];
        d.pic_sad[job] = st->pic_sad;
        if (errs)
            for (int i = 0; i < kSlots; i++) errs[i] = -1;
        if (st->pic_sad == 0) { // global_me.c:357-360: the default parameters, and nothing divides by it
            for (int i = 0; i < 6; i++) st->mat[i] = (i == 2 || i == 5) ? 1 << 16 : 0;
            st->best_error = 0;
            write_outputs(d, job, st, 0, SVT_HIP_GM_IDENTICAL);
            return;
        }
        for (int i = 0; i < 6; i++) st->mat[i] = jp->wmmat[i];
        force_wmtype(st->mat, type);
        set_candidate(st, 0, type);
        return;
    }
    if (st->done) return;
    if (launch == 1) {
        const int64_t e0 = st->run[0] ? (int64_t)w.sums[(size_t)job * kSlots] * mul : 1;
        if (errs) errs[0] = e0;
        st->best_error = e0 < jp->best_frame_error ? e0 : jp->best_frame_error;
        if (d.rfn_early_exit) { // !svt_av1_is_enough_erroradvantage(., ., GM_ERRORADV_TR_1)
            const double e = (double)st->best_error / (double)st->pic_sad;
            if (!(e < 0.50 && e * (double)jp->params_cost < 15000.0)) {
                write_outputs(d, job, st, type, SVT_HIP_GM_OK);
                return;
            }
        }
    } else {
        const int k = launch - 2, p = k % n_params; // the round the last launch held
        int       best_param = st->cur;
#pragma unroll
        for (int side = 0; side < 2; side++) {
            const int64_t e = st->run[side] ? (int64_t)w.sums[(size_t)job * kSlots + 1 + 2 * k + side] * mul : 1;
            if (errs) errs[1 + 2 * k + side] = e;
            if (e < st->best_error) { st->best_error = e; best_param = st->val[side]; }
        }
        st->mat[p] = best_param;
    }
    const int k = launch - 1; // the round of the launch to come
    if (k >= (int)d.n_refinements * n_params) {
        force_wmtype(st->mat, type);
        write_outputs(d, job, st, get_wmtype(st->mat), SVT_HIP_GM_OK);
        return;
    }
    const int p = k % n_params, step = 16 >> (k / n_params);
    st->cur = st->mat[p];
#pragma unroll
    for (int side = 0; side < 2; side++) {
        st->val[side] = add_param_offset(p, st->cur, side ? step : -step);
        st->mat[p]    = st->val[side];
        set_candidate(st, side, type);
    }
}

// ---- svt_av1_warp_error behind its shear test: launch 0 holds the first evaluation (one side), launch L >= 1 both sides of the jobs' round L - 1
__global__ __launch_bounds__(64 * kWaves) void gm_eval_kernel(const SvtHipGmRefineDesc d, const int launch) {
    __shared__ uint16_t s_src[kWaves][15 * 16];
    __shared__ uint16_t s_mid[kWaves][15 * 8];
    __shared__ uint32_t s_part[kWaves];
    const int      lane = (int)(threadIdx.x & 63u);
    const int      wave = uniform((int)(threadIdx.x >> 6));
    const uint32_t job = blockIdx.z, side = blockIdx.y;
    const Work     w   = work_of(d.work, d.n_jobs);
    const GmState *st  = w.state + job;
    if (uniform(st->run[side]) == 0) return; // the job is over or undefined, or the candidate is refused: the whole workgroup leaves

    const int pw = d.src.width, ph = d.src.height, nbx = (pw + 31) >> 5;
    int       bx, by;
    if (d.chess_refn) { // even block rows start at the second block column, odd ones at the first
        const int half = (nbx + 1) >> 1;
        by = (int)blockIdx.x / half;
        bx = ((by & 1) ? 0 : 1) + 2 * ((int)blockIdx.x % half);
        if (bx >= nbx) return;
    } else {
        by = (int)blockIdx.x / nbx;
        bx = (int)blockIdx.x % nbx;
    }
    Model m;
#pragma unroll
    for (int i = 0; i < 6; i++) m.mat[i] = uniform(st->cand_mat[side][i]);
    m.alpha = uniform(st->cand_shear[side][0]); m.beta = uniform(st->cand_shear[side][1]);
    m.gamma = uniform(st->cand_shear[side][2]); m.delta = uniform(st->cand_shear[side][3]);
    const SvtHipWarpRef r   = d.refs[d.jobs[job].ref]; // the decision kernel refused a reference outside the table
    const uint8_t      *src = origin_of(d.src);
    const uint32_t      src_stride = d.src.stride;
    const int           c = lane & 7, rr = lane >> 3;
    uint32_t            acc = 0;
#pragma unroll 1
    for (int t = wave; t < 16; t += kWaves) {
        const int jx = 32 * bx + 8 * (t & 3), iy = 32 * by + 8 * (t >> 2);
        if (jx >= pw || iy >= ph) continue; // the block is cropped to the picture; a tile that straddles the edge is computed whole
        const int v = clampi(warp_tile<false>(r, m, jx, iy, 0, 0, 11, s_src[wave], s_mid[wave], lane) - 128 - 256, 0, 255);
        const int x = jx + c, y = iy + rr;
        if (x < pw && y < ph) acc += (uint32_t)iabs(v - (int)src[(size_t)y * src_stride + (size_t)x]);
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) t += s_part[k];
        const int slot = launch == 0 ? 0 : 1 + 2 * (launch - 1) + (int)side;
        if (t) atomicAdd(w.sums + (size_t)job * kSlots + slot, (unsigned long long)t);
    }
}

// ---- correspondence_from_mvs, one workgroup per pair; the workgroup behind the last pair sums the three per-b64 arrays ----
__global__ __launch_bounds__(64 * kWaves) void gm_corr_kernel(const SvtHipGmCorrDesc d) {
    __shared__ uint32_t s_cnt[kWaves];
    __shared__ uint32_t s_sum[kWaves][3];
    const int      lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const uint32_t w64 = (d.aligned_width + 63u) >> 6, h64 = (d.aligned_height + 63u) >> 6, n_b64 = w64 * h64;
    if (blockIdx.x == d.n_pairs) {
        uint32_t sad = 0, stat = 0, gm = 0;
        for (uint32_t b = threadIdx.x; b < n_b64; b += 64 * kWaves) {
            sad += d.me.rc_me_distortion[b]; stat += d.me.stationary_block_present_sb[b]; gm += d.me.rc_me_allow_gm[b];
        }
        sad = wave_sum_dpp(sad); stat = wave_sum_dpp(stat); gm = wave_sum_dpp(gm);
        if (lane == 0) { s_sum[wave][0] = sad; s_sum[wave][1] = stat; s_sum[wave][2] = gm; }
        __syncthreads();
        if (threadIdx.x < 3) {
            uint32_t t = 0;
            for (int k = 0; k < kWaves; k++) t += s_sum[k][threadIdx.x];
            d.sums[threadIdx.x] = t;
        }
        return;
    }
    const uint32_t pair = blockIdx.x;
    const int      list = d.pairs[pair].list, ref = d.pairs[pair].ref;
    const int      bpl = 1 << d.method, bps = bpl * bpl, bsize = 64 >> d.method;
    const int      start = d.method == 0 ? 0 : (d.method == 1 ? 1 : (d.method == 2 ? 5 : 21));
    const uint32_t total = n_b64 * (uint32_t)bps, mv_slot = (uint32_t)(list ? d.max_l0 : 0) + (uint32_t)ref;
    int32_t *const out = d.corr + (size_t)pair * d.cap * 4;
    uint32_t       base = 0; // entries written so far: the same in every thread
    for (uint32_t first = 0; first < total; first += 64 * kWaves) {
        const uint32_t idx = first + threadIdx.x;
        bool           found = false;
        int            x = 0, y = 0, mvx = 0, mvy = 0;
        if (idx < total) {
            const uint32_t b64 = idx / (uint32_t)bps;
            const int      i = (int)(idx % (uint32_t)bps);
            x = (int)(b64 % w64) * 64 + (i % bpl) * bsize;
            y = (int)(b64 / w64) * 64 + (i / bpl) * bsize;
            if (x < (int)d.aligned_width && y < (int)d.aligned_height) {
                int n = start + i;
                if (!d.enable_me_8x8) { // me_idx_85_8x8_to_16x16_conversion, me_idx_16x16_to_parent_32x32_conversion as arithmetic
                    if (n >= 21) n = 5 + (((n - 21) >> 4) << 2) + (((n - 21) & 7) >> 1);
                    if (!d.enable_me_16x16 && n >= 5) n = 1 + (((n - 5) >> 3) << 1) + (((n - 5) & 3) >> 1);
                }
                const size_t   pu  = (size_t)b64 * d.n_pu + (size_t)n;
                const uint32_t cnt = d.me.total_me_candidate_index[pu] < d.max_cand ? d.me.total_me_candidate_index[pu] : d.max_cand;
                const uint8_t *cand = d.me.me_candidate_array + pu * d.max_cand;
                for (uint32_t k = 0; k < cnt && !found; k++) { // direction : 2, ref_idx_l0 : 2, ref_idx_l1 : 2, ref0_list : 1, ref1_list : 1
                    const int cd = cand[k], dir = cd & 3;
                    if (dir == 0) found = list == ((cd >> 6) & 1) && ref == ((cd >> 2) & 3);
                    else if (dir == 1) found = list == ((cd >> 7) & 1) && ref == ((cd >> 4) & 3);
                }
                if (found) {
                    const uint32_t mv = d.me.me_mv_array[pu * d.max_refs + mv_slot];
                    mvx = (int16_t)(mv & 0xFFFFu);
                    mvy = (int16_t)(mv >> 16);
                }
            }
        }
        // the compaction keeps the order: a lane's slot is the number of entries found before it
        const uint64_t ballot = __ballot(found);
        if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) { before += k < wave ? s_cnt[k] : 0; all += s_cnt[k]; }
        if (found) {
            const uint32_t slot = base + before + (uint32_t)__popcll(ballot & (((uint64_t)1 << lane) - 1));
            if (slot < d.cap) {
                out[4 * (size_t)slot] = x >> d.shift; out[4 * (size_t)slot + 1] = y >> d.shift;
                out[4 * (size_t)slot + 2] = (x + mvx) >> d.shift; out[4 * (size_t)slot + 3] = (y + mvy) >> d.shift;
            }
        }
        base += all;
        __syncthreads(); // s_cnt is written again in the next trip
    }
    if (threadIdx.x == 0) d.count[pair] = base;
}

} // namespace

extern "C" {

int svt_hip_gm_refine_check_desc(const SvtHipGmRefineDesc *d) {
    static const char who[] = "svt_hip_gm_refine_check_desc";
    if (!d) BAD("%s: null descriptor", who);
    if (!d->jobs || !d->work || !d->models || !d->best_error || !d->pic_sad || !d->status)
        BAD("%s: a mandatory pointer (jobs, work, models, best_error, pic_sad, status) is null", who);
    if (((uintptr_t)d->work & 7) != 0) BAD("%s: work is not 8-byte aligned", who);
    if (d->n_jobs > SVT_HIP_GM_MAX_JOBS) BAD("%s: n_jobs %u (0 .. %d: a grid dimension of the evaluation launch)", who, d->n_jobs, SVT_HIP_GM_MAX_JOBS);
    if (d->n_refs == 0 || d->n_refs > SVT_HIP_WARP_MAX_REFS) BAD("%s: n_refs %u (1 .. %d)", who, d->n_refs, SVT_HIP_WARP_MAX_REFS);
    if (d->n_refinements > SVT_HIP_GM_MAX_REFINEMENTS) BAD("%s: n_refinements %u (0 .. %d)", who, d->n_refinements, SVT_HIP_GM_MAX_REFINEMENTS);
    int rc = svt_hip_check_warp_refs(who, "source", &d->src, 1);
    if (!rc) rc = svt_hip_check_warp_refs(who, "reference", d->refs, d->n_refs);
    if (rc) return rc;
    for (int i = 0; i < d->n_refs; i++) {
        if (d->refs[i].width != d->src.width || d->refs[i].height != d->src.height)
            BAD("%s: reference %d: picture %u x %u, the source's is %u x %u", who, i, d->refs[i].width, d->refs[i].height, d->src.width, d->src.height);
    }
    return SVT_HIP_OK;
}

size_t svt_hip_gm_refine_work_bytes(uint32_t n_jobs) { return work_bytes(n_jobs); }

int svt_hip_gm_corr_check_desc(const SvtHipGmCorrDesc *d) {
    static const char who[] = "svt_hip_gm_corr_check_desc";
    if (!d) BAD("%s: null descriptor", who);
    if (!d->sums || (d->n_pairs && (!d->corr || !d->count))) BAD("%s: a mandatory pointer (sums; corr and count with pairs) is null", who);
    if (!d->me.total_me_candidate_index || !d->me.me_candidate_array || !d->me.me_mv_array || !d->me.rc_me_distortion || !d->me.stationary_block_present_sb ||
        !d->me.rc_me_allow_gm)
        BAD("%s: an ME result array (total_me_candidate_index, me_candidate_array, me_mv_array, rc_me_distortion, stationary_block_present_sb, rc_me_allow_gm) is null",
            who);
    if (d->aligned_width == 0 || d->aligned_height == 0) BAD("%s: aligned size %u x %u", who, d->aligned_width, d->aligned_height);
    if (d->method > 3) BAD("%s: method %u (0 .. 3)", who, d->method);
    if (d->shift > 2) BAD("%s: shift %u (0 .. 2)", who, d->shift);
    if (d->n_pairs > SVT_HIP_GM_MAX_PAIRS) BAD("%s: n_pairs %u (0 .. %d)", who, d->n_pairs, SVT_HIP_GM_MAX_PAIRS);
    if (d->enable_me_8x8 && !d->enable_me_16x16) BAD("%s: 8x8 results without 16x16 results", who);
    if (d->n_pu != svt_hip_me_n_pu(d->enable_me_16x16, d->enable_me_8x8))
        BAD("%s: n_pu %u, enable_me_16x16 %u and enable_me_8x8 %u say %u", who, d->n_pu, d->enable_me_16x16, d->enable_me_8x8,
            svt_hip_me_n_pu(d->enable_me_16x16, d->enable_me_8x8));
    if (d->max_cand == 0 || d->max_refs == 0) BAD("%s: max_cand %u, max_refs %u (non-zero)", who, d->max_cand, d->max_refs);
    const uint64_t need = ((uint64_t)1 << (2 * d->method)) * ((d->aligned_width + 63u) >> 6) * ((d->aligned_height + 63u) >> 6);
    if (d->n_pairs && d->cap < need) BAD("%s: cap %u, the picture has %llu blocks", who, d->cap, (unsigned long long)need);
    for (uint32_t i = 0; i < d->n_pairs; i++) {
        const SvtHipGmPair *p = &d->pairs[i];
        if (p->list > 1 || (unsigned)(p->list ? d->max_l0 : 0) + p->ref >= d->max_refs)
            BAD("%s: pair %u: list %u, reference %u (max_l0 %u, max_refs %u)", who, i, p->list, p->ref, d->max_l0, d->max_refs);
    }
    return SVT_HIP_OK;
}

size_t svt_hip_gm_layout(int what, int field) {
#define D(f) offsetof(SvtHipGmRefineDesc, f)
#define J(f) offsetof(SvtHipGmRefineJob, f)
#define E(f) offsetof(SvtHipGmCorrDesc, f)
#define P(f) offsetof(SvtHipGmPair, f)
    static const size_t desc[]  = {D(n_jobs), D(n_refs), D(n_refinements), D(chess_refn), D(rfn_early_exit), D(src), D(refs), D(jobs), D(work), D(models),
                                   D(best_error), D(pic_sad), D(status), D(round_error)};
    static const size_t job[]   = {J(wmmat), J(params_cost), J(ref), J(wmtype), J(reserved), J(best_frame_error)};
    static const size_t cdesc[] = {E(aligned_width), E(aligned_height), E(enable_me_8x8), E(enable_me_16x16), E(max_cand), E(max_refs), E(max_l0), E(n_pu),
                                   E(method), E(shift), E(n_pairs), E(cap), E(pairs), E(me), E(corr), E(count), E(sums)};
    static const size_t pair[]  = {P(list), P(ref), P(reserved)};
#undef D
#undef J
#undef E
#undef P
    const SvtHipLayoutRow rows[] = {layout_row<SvtHipGmRefineDesc>(desc), layout_row<SvtHipGmRefineJob>(job), layout_row<SvtHipGmCorrDesc>(cdesc),
                                    layout_row<SvtHipGmPair>(pair)};
    return layout_lookup(rows, what, field);
}

int svt_hip_gm_refine_batch(SvtHipContext *ctx, const SvtHipGmRefineDesc *d) {
    return enqueue_batch("svt_hip_gm_refine_batch", ctx, d, svt_hip_gm_refine_check_desc, &SvtHipGmRefineDesc::n_jobs, [=] {
        const uint32_t pw = d->src.width, ph = d->src.height, nbx = ceil_div(pw, 32), nby = ceil_div(ph, 32);
        const uint32_t blocks = (d->chess_refn ? (nbx + 1) / 2 : nbx) * nby; // 32x32 blocks an evaluation may select
        const int      rounds = 6 * (int)d->n_refinements;                    // the most a job can have
        const dim3     decide(ceil_div(d->n_jobs, 64));
        (void)hipMemsetAsync(d->work, 0, work_bytes(d->n_jobs), ctx->stream);
        hipLaunchKernelGGL(gm_sad_kernel, dim3(ceil_div(ph, kSadRows), d->n_refs), dim3(64 * kWaves), 0, ctx->stream, *d);
        for (int launch = 0; launch <= rounds; launch++) {
            hipLaunchKernelGGL(gm_decide_kernel, decide, dim3(64), 0, ctx->stream, *d, launch);
            hipLaunchKernelGGL(gm_eval_kernel, dim3(blocks, launch ? 2 : 1, d->n_jobs), dim3(64 * kWaves), 0, ctx->stream, *d, launch);
        }
        hipLaunchKernelGGL(gm_decide_kernel, decide, dim3(64), 0, ctx->stream, *d, rounds + 1);
    });
}

int svt_hip_gm_correspondence_batch(SvtHipContext *ctx, const SvtHipGmCorrDesc *d) {
    if (!ctx || !d) BAD("svt_hip_gm_correspondence_batch: null context or descriptor");
    const int rc = svt_hip_gm_corr_check_desc(d);
    if (rc) return rc;
    return enqueue_locked("svt_hip_gm_correspondence_batch", ctx,
                          [=] { hipLaunchKernelGGL(gm_corr_kernel, dim3(d->n_pairs + 1), dim3(64 * kWaves), 0, ctx->stream, *d); });
}

} // extern "C"
