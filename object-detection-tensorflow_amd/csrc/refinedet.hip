// RefineDet box side (reference RefineDet.py:422-567 loss, :189-206 decode): the two-stage ARM -> ODM loss with both gradients, and the
// two-stage decode.  Matching is RetinaNet's (odtk_retina_match: best anchor per box, positive > 0.5, negative < 0.4), the ARM's hard negatives are
// mined by the SSD300 path (odtk_softmax_ce_const -> odtk_nms_batched); this file adds what is new: one pass over the positive rows and the mined
// negatives that evaluates six loss terms and scatters four gradients.  Latency-bound (a few thousand rows per image): LOSS_SPLIT workgroups per
// image, fixed-order partial sums (deterministic loss), float atomics only for the gradients (duplicate best anchors hit one row twice).
// ODM rows of up to RD_MAXC = 96 logits belong to one thread; rows of 97 .. wr::MAXC = 256 logits to a 16-lane group (wide_row.h), in kernels of their own
// at the end of each half of this file.  The host picks by C; the one-thread kernels and their launch geometry are those of the versions before 108.
#include "common.h"
#include "wide_row.h"

namespace odtk {
namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_SPLIT = 8;
constexpr int RD_MAXC = 96;

__device__ __forceinline__ float rd_block_sum(float v, float* sm) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < RD_THREADS / 64; ++i) t += sm[i];
    return t;
}

struct RdArgs {
    const float* arm_loc; const float* arm_conf; const float* odm_loc; const float* odm_conf;
    int N, A, C;
    const float* yx; const float* hw; const float* gt; int P;
    const int* ngt; const int* best; const unsigned char* status; const int* rgindex; const int* counts;
    const float* negloss; const int* sel_idx; int sel_cap; const int* sel_cnt;
    float grad_scale;
    float* loss_parts;                       // [N][8]: neg_arm, pos_armconf, pos_coord_arm, neg_odm, pos_odmconf, pos_coord_odm, total, #odm negatives
    float* d_arm_loc; float* d_arm_conf; float* d_odm_loc; float* d_odm_conf;
    float* parts;                            // [N][RD_SPLIT][8]
};

__device__ __forceinline__ float sl1(float d) { const float a = fabsf(d); return a < 1.f ? 0.5f * d * d : a - 0.5f; }
__device__ __forceinline__ float sl1g(float d) { return fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f); }

// softmax cross entropy of row z [C] against `label`; adds (softmax - onehot) * g to dz
__device__ __forceinline__ float ce_row(const float* z, float* dz, int C, int label, float g) {
    float m = z[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    float e[RD_MAXC];
    float s = 0.f;
    for (int c = 0; c < C; ++c) { e[c] = expf(z[c] - m); s += e[c]; }
    for (int c = 0; c < C; ++c) atomicAdd(dz + c, (e[c] / s - (c == label ? 1.f : 0.f)) * g);
    return logf(s) - (z[label] - m);
}

// the two smooth-L1 terms of a positive row and their gradients (RefineDet.py:541-563): they do not read the class logits
__device__ __forceinline__ void rd_positive_boxes(const RdArgs& k, size_t row, int a, const float* gb, float gsc, float& armx, float& odmx) {
    const float* al = k.arm_loc + row * 4;
    const float* ol = k.odm_loc + row * 4;
    float* dal = k.d_arm_loc + row * 4;
    float* dol = k.d_odm_loc + row * 4;
    float ax = 0.f, ox = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float ayx = k.yx[2 * a + j], ahw = k.hw[2 * a + j];
        const float gyx = gb[j], ghw = gb[2 + j];
        // ARM box loss against the anchor
        const float d_yx = al[j] - (gyx - ayx) / ahw;
        const float d_hw = al[2 + j] - logf(ghw / ahw);
        ax += sl1(d_yx) + sl1(d_hw);
        float g_ayx = sl1g(d_yx), g_ahw = sl1g(d_hw);
        // ODM box loss against the ARM-refined anchor (no stop_gradient in the reference: the targets depend on the ARM outputs)
        const float ryx = al[j] * ahw + ayx;
        const float rhw = expf(al[2 + j]) * ahw;
        const float oyx = (gyx - ryx) / rhw;
        const float e_yx = ol[j] - oyx;
        const float e_hw = ol[2 + j] - logf(ghw / rhw);
        ox += sl1(e_yx) + sl1(e_hw);
        const float s_yx = sl1g(e_yx), s_hw = sl1g(e_hw);
        atomicAdd(dol + j, s_yx * gsc);
        atomicAdd(dol + 2 + j, s_hw * gsc);
        g_ayx += s_yx * (ahw / rhw);                       // d(-oyx)/d(arm_yx) = ahw / rhw
        g_ahw += s_yx * oyx + s_hw;                        // d(-oyx)/d(arm_hw) = oyx;  d(-log(ghw / rhw))/d(arm_hw) = 1
        atomicAdd(dal + j, g_ayx * gsc);
        atomicAdd(dal + 2 + j, g_ahw * gsc);
    }
    armx += ax; odmx += ox;
}

// one row of the positive set: anchor `a`, ground-truth box `g` (RefineDet.py:505-563)
__device__ __forceinline__ void rd_positive(const RdArgs& k, int n, int a, int g, float gsc, float& armc, float& armx, float& odmc, float& odmx) {
    const size_t row = (size_t)n * k.A + a;
    const float* gb = k.gt + ((size_t)n * k.P + g) * 5;
    armc += ce_row(k.arm_conf + row * 2, k.d_arm_conf + row * 2, 2, 0, gsc);                       // ARM: class 0 = object
    odmc += ce_row(k.odm_conf + row * k.C, k.d_odm_conf + row * k.C, k.C, (int)gb[4], gsc);
    rd_positive_boxes(k, row, a, gb, gsc, armx, odmx);
}

__global__ void __launch_bounds__(RD_THREADS) refinedet_loss_kernel(const RdArgs k) {
    __shared__ float sm[RD_THREADS / 64];
    __shared__ float s_nodm;
    const int n = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int G = k.ngt[n], num_pos = k.counts[n * 4 + 0], nsel = k.sel_cnt[n], bg = k.C - 1;
    float neg_arm = 0.f, neg_odm = 0.f, nodm = 0.f;
    if (s == 0) {
        // the mined ARM negatives (a few hundred rows): ARM cross entropy against class 1, and -- for those whose ARM background LOGIT is below
        // 0.99 (sic, RefineDet.py:535) -- ODM cross entropy against the background class; the ODM mean needs the count first
        for (int i = tid; i < nsel; i += RD_THREADS) {
            const int a = k.sel_idx[(size_t)n * k.sel_cap + i];
            if (k.arm_conf[((size_t)n * k.A + a) * 2 + 1] < 0.99f) nodm += 1.f;
        }
        nodm = rd_block_sum(nodm, sm);
        if (tid == 0) s_nodm = nodm;
        __syncthreads();
        const float g_arm = k.grad_scale / (float)nsel, g_odm = k.grad_scale / s_nodm;
        for (int i = tid; i < nsel; i += RD_THREADS) {
            const int a = k.sel_idx[(size_t)n * k.sel_cap + i];
            const size_t row = (size_t)n * k.A + a;
            neg_arm += ce_row(k.arm_conf + row * 2, k.d_arm_conf + row * 2, 2, 1, g_arm);
            if (k.arm_conf[row * 2 + 1] < 0.99f) neg_odm += ce_row(k.odm_conf + row * k.C, k.d_odm_conf + row * k.C, k.C, bg, g_odm);
        }
    }
    float armc = 0.f, armx = 0.f, odmc = 0.f, odmx = 0.f;
    const float gsc = k.grad_scale / (float)num_pos;
    if (s == 0)
        for (int g = tid; g < G; g += RD_THREADS) rd_positive(k, n, k.best[(size_t)n * k.P + g], g, gsc, armc, armx, odmc, odmx);
    const int per = (k.A + RD_SPLIT - 1) / RD_SPLIT;
    const int a1 = min(k.A, (s + 1) * per);
    for (int a = s * per + tid; a < a1; a += RD_THREADS)
        if (k.status[(size_t)n * k.A + a] == 1) rd_positive(k, n, a, k.rgindex[(size_t)n * k.A + a], gsc, armc, armx, odmc, odmx);
    float v[7] = {neg_arm, armc, armx, neg_odm, odmc, odmx, 0.f};
    for (int i = 0; i < 6; ++i) v[i] = rd_block_sum(v[i], sm);
    if (tid == 0) {
        float* o = k.parts + ((size_t)n * RD_SPLIT + s) * 8;
        for (int i = 0; i < 6; ++i) o[i] = v[i];
        o[6] = s == 0 ? s_nodm : 0.f;
    }
}

// ---- ODM rows of 97 .. wr::MAXC logits: refinedet_loss_kernel with a 16-lane group where it has a thread.  Same grid, same three row sets, same k.parts and
// the same refinedet_loss_final_kernel behind it.  Group q of 16 takes every 16th row where thread q of 256 takes every 256th.  The loops have trip counts
// that are uniform in the workgroup and switch rows off with `on`: every lane reaches every shuffle.  What does not read the ODM logits -- the two-logit ARM
// cross entropy, the smooth-L1 terms -- is the scalar code of the one-thread kernel, run by the group's first lane, which alone adds the row to the sums.
constexpr int RD_GROUPS = RD_THREADS / wr::L;

// ce_row for the ARM's two logits, without the array
__device__ __forceinline__ float ce_row2(const float* z, float* dz, int label, float g) {
    const float z0 = z[0], z1 = z[1];
    const float m = fmaxf(z0, z1);
    const float e0 = expf(z0 - m), e1 = expf(z1 - m);
    const float s = e0 + e1;
    atomicAdd(dz, (e0 / s - (label == 0 ? 1.f : 0.f)) * g);
    atomicAdd(dz + 1, (e1 / s - (label == 1 ? 1.f : 0.f)) * g);
    return logf(s) - ((label == 0 ? z0 : z1) - m);
}

// ce_row for a group: lane j adds (softmax - onehot) * g to its classes of dz (ADDS: a row can be visited twice); the row's loss in every lane, 0 if off
template <int K>
__device__ __forceinline__ float ce_row_wide(const float* z, float* dz, int C, int label, float g, int j, bool on) {
    float v[K], m, s;
    wr::load<K>(z, C, j, on, v);
    wr::softmax<K>(v, C, j, on, m, s);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int c = j + wr::L * i;
        if (on && c < C) atomicAdd(dz + c, (v[i] / s - (c == label ? 1.f : 0.f)) * g);
    }
    return on ? logf(s) - (z[label] - m) : 0.f;
}

template <int K>
__device__ __forceinline__ void rd_positive_wide(const RdArgs& k, int n, int a, int g, float gsc, int j, bool on, float& armc, float& armx, float& odmc,
                                                 float& odmx) {
    const size_t row = (size_t)n * k.A + a;
    const float* gb = k.gt + ((size_t)n * k.P + g) * 5;
    const float ce = ce_row_wide<K>(k.odm_conf + row * k.C, k.d_odm_conf + row * k.C, k.C, on ? (int)gb[4] : 0, gsc, j, on);
    if (!on || j != 0) return;
    armc += ce_row2(k.arm_conf + row * 2, k.d_arm_conf + row * 2, 0, gsc);
    odmc += ce;
    rd_positive_boxes(k, row, a, gb, gsc, armx, odmx);
}

template <int K>
__global__ void __launch_bounds__(RD_THREADS) refinedet_loss_wide_kernel(const RdArgs k) {
    __shared__ float sm[RD_THREADS / 64];
    __shared__ float s_nodm;
    const int n = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, j = tid & (wr::L - 1), q = tid / wr::L;
    const int G = k.ngt[n], num_pos = k.counts[n * 4 + 0], nsel = k.sel_cnt[n], bg = k.C - 1;
    float neg_arm = 0.f, neg_odm = 0.f, nodm = 0.f;
    if (s == 0) {
        for (int i = tid; i < nsel; i += RD_THREADS) {            // the count first, a thread per row as in refinedet_loss_kernel
            const int a = k.sel_idx[(size_t)n * k.sel_cap + i];
            if (k.arm_conf[((size_t)n * k.A + a) * 2 + 1] < 0.99f) nodm += 1.f;
        }
        nodm = rd_block_sum(nodm, sm);
        if (tid == 0) s_nodm = nodm;
        __syncthreads();
        const float g_arm = k.grad_scale / (float)nsel, g_odm = k.grad_scale / s_nodm;
        for (int i0 = 0; i0 < nsel; i0 += RD_GROUPS) {
            const int i = i0 + q;
            const bool on = i < nsel;
            const int a = on ? k.sel_idx[(size_t)n * k.sel_cap + i] : 0;
            const size_t row = (size_t)n * k.A + a;
            const bool odm = on && k.arm_conf[row * 2 + 1] < 0.99f;
            const float ce = ce_row_wide<K>(k.odm_conf + row * k.C, k.d_odm_conf + row * k.C, k.C, bg, g_odm, j, odm);
            if (on && j == 0) {
                neg_arm += ce_row2(k.arm_conf + row * 2, k.d_arm_conf + row * 2, 1, g_arm);
                if (odm) neg_odm += ce;
            }
        }
    }
    float armc = 0.f, armx = 0.f, odmc = 0.f, odmx = 0.f;
    const float gsc = k.grad_scale / (float)num_pos;
    if (s == 0)
        for (int g0 = 0; g0 < G; g0 += RD_GROUPS) {
            const int g = g0 + q;
            const bool on = g < G;
            rd_positive_wide<K>(k, n, on ? k.best[(size_t)n * k.P + g] : 0, on ? g : 0, gsc, j, on, armc, armx, odmc, odmx);
        }
    const int per = (k.A + RD_SPLIT - 1) / RD_SPLIT;
    const int a1 = min(k.A, (s + 1) * per);
    for (int r0 = s * per; r0 < a1; r0 += RD_GROUPS) {
        const int a = r0 + q;
        const bool on = a < a1 && k.status[(size_t)n * k.A + a] == 1;
        if (!__any(on)) continue;                                  // (uniform in the wave, and the shuffles stay inside it)
        rd_positive_wide<K>(k, n, on ? a : 0, on ? k.rgindex[(size_t)n * k.A + a] : 0, gsc, j, on, armc, armx, odmc, odmx);
    }
    float v[6] = {neg_arm, armc, armx, neg_odm, odmc, odmx};
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = rd_block_sum(v[i], sm);
    if (tid == 0) {
        float* o = k.parts + ((size_t)n * RD_SPLIT + s) * 8;
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = v[i];
        o[6] = s == 0 ? s_nodm : 0.f;
    }
}

__global__ void __launch_bounds__(64) refinedet_loss_final_kernel(const RdArgs k) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= k.N) return;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < RD_SPLIT; ++s)
        for (int i = 0; i < 7; ++i) t[i] += k.parts[((size_t)n * RD_SPLIT + s) * 8 + i];
    const float np_ = (float)k.counts[n * 4 + 0], ns = (float)k.sel_cnt[n];
    float* o = k.loss_parts + (size_t)n * 8;
    o[0] = t[0] / ns; o[1] = t[1] / np_; o[2] = t[2] / np_;            // means of empty sets -> NaN, as TensorFlow
    o[3] = t[3] / t[6]; o[4] = t[4] / np_; o[5] = t[5] / np_;
    o[6] = (o[0] + o[1] + o[2]) + (o[3] + o[4] + o[5]);
    o[7] = t[6];
}

// RefineDet.py:189-206: one thread per anchor, blockIdx.y = image: its four prediction tensors start row_istride rows behind those of the image before,
// the outputs are [N][A][..]; the anchors are shared
__global__ void refinedet_decode_kernel(const float* __restrict__ arm_loc, const float* __restrict__ arm_conf, const float* __restrict__ odm_loc,
                                        const float* __restrict__ odm_conf, long long row_istride, int A, int C, const float* __restrict__ yx,
                                        const float* __restrict__ hw, float thr, float* __restrict__ conf, float* __restrict__ boxes,
                                        unsigned char* __restrict__ keep, unsigned char* __restrict__ cand) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= A) return;
    const size_t img = blockIdx.y, in0 = img * (size_t)row_istride, out0 = img * (size_t)A;
    arm_loc += in0 * 4; arm_conf += in0 * 2; odm_loc += in0 * 4; odm_conf += in0 * C;
    conf += out0 * (C - 1); boxes += out0 * 4; keep += out0; cand += out0 * (C - 1);
    const float z0 = arm_conf[2 * a], z1 = arm_conf[2 * a + 1];
    const float am = fmaxf(z0, z1);
    const float e0 = expf(z0 - am), e1 = expf(z1 - am);
    const bool arm_ok = e1 / (e0 + e1) < 0.99f;
    const float* z = odm_conf + (size_t)a * C;
    float m = z[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    float e[RD_MAXC];
    float s = 0.f;
    for (int c = 0; c < C; ++c) { e[c] = expf(z[c] - m); s += e[c]; }
    int arg = 0; float best = -1.f;
    for (int c = 0; c < C; ++c) {
        const float p = e[c] / s;
        e[c] = p;
        if (p > best) { best = p; arg = c; }
    }
    const bool kp = arm_ok && arg < C - 1;
    keep[a] = kp ? 1 : 0;
    for (int c = 0; c < C - 1; ++c) {
        conf[(size_t)a * (C - 1) + c] = e[c];
        cand[(size_t)a * (C - 1) + c] = (kp && e[c] >= thr) ? 1 : 0;
    }
    const float* al = arm_loc + (size_t)a * 4;
    const float* ol = odm_loc + (size_t)a * 4;
    float lo[2], hi[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float ayx = yx[2 * a + j], ahw = hw[2 * a + j];
        const float ryx = al[j] * ahw + ayx;
        const float rhw = expf(al[2 + j]) * ahw;
        const float oyx = ol[j] * rhw + ryx;
        const float ohw = expf(ol[2 + j]) * rhw;
        lo[j] = oyx - ohw / 2.f; hi[j] = oyx + ohw / 2.f;
    }
    boxes[4 * a + 0] = lo[0]; boxes[4 * a + 1] = lo[1]; boxes[4 * a + 2] = hi[0]; boxes[4 * a + 3] = hi[1];
}

// refinedet_decode_kernel for ODM rows of 97 .. wr::MAXC logits: a 16-lane group per anchor, 16 anchors per workgroup.  The ARM test is per row: every lane
// of the group evaluates it from the same two logits with the statements above (the same bits); the box is the first lane's, in the arithmetic above.
constexpr int RD_DECODE_WIDE_THREADS = 256;
template <int K>
__global__ void __launch_bounds__(RD_DECODE_WIDE_THREADS) refinedet_decode_wide_kernel(
    const float* __restrict__ arm_loc, const float* __restrict__ arm_conf, const float* __restrict__ odm_loc, const float* __restrict__ odm_conf,
    long long row_istride, int A, int C, const float* __restrict__ yx, const float* __restrict__ hw, float thr, float* __restrict__ conf,
    float* __restrict__ boxes, unsigned char* __restrict__ keep, unsigned char* __restrict__ cand) {
    const int j = threadIdx.x & (wr::L - 1);
    const int r = blockIdx.x * (RD_DECODE_WIDE_THREADS / wr::L) + threadIdx.x / wr::L;
    const bool on = r < A;
    const int a = on ? r : A - 1;
    const size_t img = blockIdx.y, in0 = img * (size_t)row_istride, out0 = img * (size_t)A;
    arm_loc += in0 * 4; arm_conf += in0 * 2; odm_loc += in0 * 4; odm_conf += in0 * C;
    conf += out0 * (C - 1); boxes += out0 * 4; keep += out0; cand += out0 * (C - 1);
    float v[K], m, s;
    wr::load<K>(odm_conf + (size_t)a * C, C, j, on, v);
    wr::softmax<K>(v, C, j, on, m, s);
    int arg = 0; float best = -1.f;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int c = j + wr::L * i;
        if (c < C) {
            const float p = v[i] / s;
            v[i] = p;
            if (p > best) { best = p; arg = c; }                   // the lane's first maximum
        }
    }
    wr::group_argmax(best, arg);                                   // the lowest index among equal maxima: `p > best` over ascending c
    if (!on) return;
    const float z0 = arm_conf[2 * a], z1 = arm_conf[2 * a + 1];
    const float am = fmaxf(z0, z1);
    const float e0 = expf(z0 - am), e1 = expf(z1 - am);
    const bool arm_ok = e1 / (e0 + e1) < 0.99f;
    const bool kp = arm_ok && arg < C - 1;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int c = j + wr::L * i;
        if (c < C - 1) {
            conf[(size_t)a * (C - 1) + c] = v[i];
            cand[(size_t)a * (C - 1) + c] = (kp && v[i] >= thr) ? 1 : 0;
        }
    }
    if (j != 0) return;
    keep[a] = kp ? 1 : 0;
    const float* al = arm_loc + (size_t)a * 4;
    const float* ol = odm_loc + (size_t)a * 4;
    float lo[2], hi[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float ayx = yx[2 * a + i], ahw = hw[2 * a + i];
        const float ryx = al[i] * ahw + ayx;
        const float rhw = expf(al[2 + i]) * ahw;
        const float oyx = ol[i] * rhw + ryx;
        const float ohw = expf(ol[2 + i]) * rhw;
        lo[i] = oyx - ohw / 2.f; hi[i] = oyx + ohw / 2.f;
    }
    boxes[4 * a + 0] = lo[0]; boxes[4 * a + 1] = lo[1]; boxes[4 * a + 2] = hi[0]; boxes[4 * a + 3] = hi[1];
}

static float* g_rd_scratch[16];
constexpr int RD_SCRATCH_IMAGES = 4096;

}  // namespace
}  // namespace odtk

using namespace odtk;

extern "C" int odtk_refinedet_loss(const float* arm_loc, const float* arm_conf, const float* odm_loc, const float* odm_conf, int N, int A, int C,
                                   const float* yx, const float* hw, const float* gt, int P, const int* ngt, const int* best,
                                   const unsigned char* status, const int* rgindex, const int* counts, const float* negloss, const int* sel_idx,
                                   int sel_cap, const int* sel_cnt, float grad_scale, float* loss_parts, float* d_arm_loc, float* d_arm_conf,
                                   float* d_odm_loc, float* d_odm_conf, void* stream) {
    ODTK_REQUIRE(arm_loc && arm_conf && odm_loc && odm_conf && yx && hw && gt && ngt && best && status && rgindex && counts && negloss && sel_idx &&
                 sel_cnt && loss_parts && d_arm_loc && d_arm_conf && d_odm_loc && d_odm_conf, "refinedet_loss: null pointer");
    ODTK_REQUIRE(N > 0 && N <= RD_SCRATCH_IMAGES && A > 0 && P > 0, "refinedet_loss: N=%d A=%d P=%d out of range", N, A, P);
    ODTK_REQUIRE(C > 1 && C <= wr::MAXC, "refinedet_loss: C=%d unsupported (2 <= C <= %d)", C, wr::MAXC);
    int dev = 0;
    ODTK_CHECK_HIP(hipGetDevice(&dev));
    ODTK_REQUIRE(dev >= 0 && dev < 16, "refinedet_loss: device %d unsupported", dev);
    if (!g_rd_scratch[dev]) ODTK_CHECK_HIP(hipMalloc((void**)&g_rd_scratch[dev], (size_t)RD_SCRATCH_IMAGES * RD_SPLIT * 8 * sizeof(float)));
    hipStream_t st = (hipStream_t)stream;
    if (int e = zero_async(d_arm_loc, (size_t)N * A * 4 * sizeof(float), st)) return e;
    if (int e = zero_async(d_arm_conf, (size_t)N * A * 2 * sizeof(float), st)) return e;
    if (int e = zero_async(d_odm_loc, (size_t)N * A * 4 * sizeof(float), st)) return e;
    if (int e = zero_async(d_odm_conf, (size_t)N * A * C * sizeof(float), st)) return e;
    RdArgs k;
    k.arm_loc = arm_loc; k.arm_conf = arm_conf; k.odm_loc = odm_loc; k.odm_conf = odm_conf; k.N = N; k.A = A; k.C = C;
    k.yx = yx; k.hw = hw; k.gt = gt; k.P = P; k.ngt = ngt; k.best = best; k.status = status; k.rgindex = rgindex; k.counts = counts;
    k.negloss = negloss; k.sel_idx = sel_idx; k.sel_cap = sel_cap; k.sel_cnt = sel_cnt; k.grad_scale = grad_scale;
    k.loss_parts = loss_parts; k.d_arm_loc = d_arm_loc; k.d_arm_conf = d_arm_conf; k.d_odm_loc = d_odm_loc; k.d_odm_conf = d_odm_conf;
    k.parts = g_rd_scratch[dev];
    if (C <= RD_MAXC) hipLaunchKernelGGL(refinedet_loss_kernel, dim3(N, RD_SPLIT), dim3(RD_THREADS), 0, st, k);
    else if (C <= 8 * wr::L) hipLaunchKernelGGL(refinedet_loss_wide_kernel<8>, dim3(N, RD_SPLIT), dim3(RD_THREADS), 0, st, k);   // 97 .. 128 logits
    else hipLaunchKernelGGL(refinedet_loss_wide_kernel<16>, dim3(N, RD_SPLIT), dim3(RD_THREADS), 0, st, k);                     // 129 .. 256
    hipLaunchKernelGGL(refinedet_loss_final_kernel, dim3((N + 63) / 64), dim3(64), 0, st, k);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}

// the decode launch of N images (csrc/detect_batched.hip: odtk_refinedet_decode_batched)
int odtk::refinedet_decode_launch(const float* arm_loc, const float* arm_conf, const float* odm_loc, const float* odm_conf, long long row_istride, int N,
                                  int A, int C, const float* yx, const float* hw, float score_threshold, float* conf, float* boxes, unsigned char* keep,
                                  unsigned char* cand, void* stream) {
    ODTK_REQUIRE(A > 0, "refinedet_decode: A=%d out of range", A);
    ODTK_REQUIRE(C > 1 && C <= wr::MAXC, "refinedet_decode: C=%d unsupported (2 <= C <= %d)", C, wr::MAXC);
    if (C <= RD_MAXC) {
        hipLaunchKernelGGL(refinedet_decode_kernel, dim3((A + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, arm_loc, arm_conf, odm_loc, odm_conf,
                           row_istride, A, C, yx, hw, score_threshold, conf, boxes, keep, cand);
    } else {                                                 // 97 .. wr::MAXC logits: a 16-lane group per anchor, 8 or 16 registers per lane
        const dim3 grid(ceil_div(A, RD_DECODE_WIDE_THREADS / wr::L), N), block(RD_DECODE_WIDE_THREADS);
        if (C <= 8 * wr::L)
            hipLaunchKernelGGL(refinedet_decode_wide_kernel<8>, grid, block, 0, (hipStream_t)stream, arm_loc, arm_conf, odm_loc, odm_conf, row_istride, A, C,
                               yx, hw, score_threshold, conf, boxes, keep, cand);
        else
            hipLaunchKernelGGL(refinedet_decode_wide_kernel<16>, grid, block, 0, (hipStream_t)stream, arm_loc, arm_conf, odm_loc, odm_conf, row_istride, A, C,
                               yx, hw, score_threshold, conf, boxes, keep, cand);
    }
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}

extern "C" int odtk_refinedet_decode(const float* arm_loc, const float* arm_conf, const float* odm_loc, const float* odm_conf, int A, int C,
                                     const float* yx, const float* hw, float score_threshold, float* conf, float* boxes, unsigned char* keep,
                                     unsigned char* cand, void* stream) {
    ODTK_REQUIRE(arm_loc && arm_conf && odm_loc && odm_conf && yx && hw && conf && boxes && keep && cand, "refinedet_decode: null pointer");
    return refinedet_decode_launch(arm_loc, arm_conf, odm_loc, odm_conf, 0, 1, A, C, yx, hw, score_threshold, conf, boxes, keep, cand, stream);
}
