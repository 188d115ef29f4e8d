// Soft-NMS (Bodla et al. 2017: linear and Gaussian score decay) behind the batched inference tail, and the detection pack that takes its decayed scores.
// One workgroup per (image, class) problem.  The live scores sit in LDS and every entry has ONE owner thread (entry e belongs to thread e % 1024), which is the
// only one that ever writes it: a pick is a block arg-max over the owners' entries (64-bit keys: sortable score, then the lower row first; wave64 shuffles, one
// LDS stage of 16 keys, double-buffered so that a pick costs a single barrier) followed by the owners' decay pass.  No atomics, a fixed reduction order: two
// runs give identical bytes.  The `hard` method (0) is greedy NMS in this form and picks what odtk_nms_image_class picks.
//   * up to SOFT_CAP live rows: (row index, score, normalised box) compacted into LDS in row order (ballot + scan, as compact_rows_kernel), 24 B per row,
//     48 KiB -- the decay pass touches LDS only;
//   * more live rows than that: the slow path.  score[n] (4 B per row, 128 KiB at n = 32768, dead rows at -inf) takes the place of the compacted rows, a pick
//     scans all n entries and the decay pass reads the boxes of the live rows from global memory.  No row is ever dropped.
#include "common.h"
#include "nms_iou.h"

namespace odtk {
namespace {

using nms_iou::NBox;
using nms_iou::norm_box;
using nms_iou::iou_nms;

constexpr int SOFT_THREADS = 1024;
constexpr int SOFT_WAVES = SOFT_THREADS / 64;
constexpr int SOFT_CAP = 2048;                  // live rows of a problem kept compacted in LDS

struct SoftArgs {
    const float* boxes; long long box_istride;
    const float* scores; long long score_istride, score_cstride; int score_estride;
    const unsigned char* valid; long long valid_istride, valid_cstride; int valid_estride, valid_value;
    int n; const int* n_dev; int nc;
    int max_out, method;
    float thr, sigma, min_score;
    int* out_idx; float* out_score; int cap; int* out_cnt;
};

// the order of nms_kernel's keys: score descending, then the lower row
__device__ __forceinline__ unsigned sortable(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unsortable(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// score[e], e < cnt: the live scores (-inf = dead).  FULL: e is the row itself and its box is read from `boxes`; otherwise e is a compacted position, its row
// cidx[e] and its box cbox[e].  Whole workgroups enter and leave together (every thread sees the same keys).
template <bool FULL>
__device__ __forceinline__ void soft_pick_loop(const SoftArgs& a, int b, int mo, int cnt, float* score, const int* cidx, const NBox* cbox, const float* boxes,
                                               unsigned long long (*s_best)[SOFT_WAVES]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int count = 0;
    for (; count < mo; ++count) {
        unsigned long long best = 0ull;
        for (int e = tid; e < cnt; e += SOFT_THREADS) {
            const float s = score[e];
            if (s > -INFINITY) {
                const unsigned long long key = ((unsigned long long)sortable(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)e);
                best = key > best ? key : best;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(best, o);
            best = other > best ? other : best;
        }
        if (lane == 0) s_best[count & 1][wave] = best;
        __syncthreads();
        best = 0ull;
        for (int w = 0; w < SOFT_WAVES; ++w) {
            const unsigned long long v = s_best[count & 1][w];
            best = v > best ? v : best;
        }
        if (best == 0ull) break;                                                // no live row
        const int m = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));
        const int row = FULL ? m : cidx[m];
        NBox bm;
        if (FULL) {
            const float4 raw = *reinterpret_cast<const float4*>(boxes + (size_t)row * 4);
            bm = norm_box(raw.x, raw.y, raw.z, raw.w);
        } else {
            bm = cbox[m];
        }
        if (tid == 0) {
            a.out_idx[(size_t)b * a.cap + count] = row;
            a.out_score[(size_t)b * a.cap + count] = unsortable((unsigned)(best >> 32));
        }
        for (int e = tid; e < cnt; e += SOFT_THREADS) {                         // the owner's entries: nobody else reads or writes them
            float s = score[e];
            if (e == m) s = -INFINITY;
            if (!(s > -INFINITY)) { score[e] = s; continue; }
            NBox bj;
            if (FULL) {
                const float4 raw = *reinterpret_cast<const float4*>(boxes + (size_t)e * 4);
                bj = norm_box(raw.x, raw.y, raw.z, raw.w);
            } else {
                bj = cbox[e];
            }
            const float iou = iou_nms(bm, bj);
            if (a.method == 0) {
                if (iou > a.thr) s = -INFINITY;
            } else {
                if (a.method == 1) {
                    if (iou > a.thr) s = s * (1.f - iou);
                } else {
                    s = s * expf(-(iou * iou) / a.sigma);
                }
                if (!(s >= a.min_score)) s = -INFINITY;                         // below min_score (or NaN): dead
            }
            score[e] = s;
        }
    }
    if (tid == 0) a.out_cnt[b] = count;
}

__global__ void __launch_bounds__(SOFT_THREADS) soft_nms_kernel(const SoftArgs a) {
    extern __shared__ __attribute__((aligned(16))) char soft_lds[];
    __shared__ int s_wave[SOFT_WAVES];
    __shared__ unsigned long long s_best[2][SOFT_WAVES];
    const int b = blockIdx.x, img = b / a.nc, c = b % a.nc, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* boxes = a.boxes + (long long)img * a.box_istride;
    const float* scores = a.scores + (long long)img * a.score_istride + (long long)c * a.score_cstride;
    const unsigned char* valid = a.valid ? a.valid + (long long)img * a.valid_istride + (long long)c * a.valid_cstride : nullptr;
    const int n_eff = a.n_dev ? min(a.n, max(a.n_dev[img], 0)) : a.n;
    int mo = a.max_out < a.cap ? a.max_out : a.cap;
    if (mo < 0) mo = 0;
    // nms_kernel's rule: the row is valid and its score is above -inf (NaN excluded)
    auto live = [&](int i, float& s) -> bool {
        bool ok = true;
        if (valid) ok = valid[(long long)i * a.valid_estride] == (unsigned char)a.valid_value;
        s = scores[(long long)i * a.score_estride];
        return ok && s > -INFINITY;
    };
    const int capc = a.n < SOFT_CAP ? a.n : SOFT_CAP;
    NBox* cbox = reinterpret_cast<NBox*>(soft_lds);                             // [capc]
    float* cscore = reinterpret_cast<float*>(soft_lds + (size_t)capc * 16);     // [capc]
    int* cidx = reinterpret_cast<int*>(soft_lds + (size_t)capc * 20);           // [capc]
    // the live rows in row order, 1024 at a time: rank = the passes before + the waves before (LDS) + the lanes before (ballot); `done` ends as the TRUE count
    int done = 0;
    if (mo > 0) {
        for (int i0 = 0; i0 < n_eff; i0 += SOFT_THREADS) {                      // (whole workgroups enter: ballots and barriers need every thread)
            const int i = i0 + tid;
            float s = 0.f;
            const bool flag = i < n_eff && live(i, s);
            const unsigned long long mask = __ballot(flag);
            if (lane == 0) s_wave[wave] = __popcll(mask);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < SOFT_WAVES; ++w) {
                const int v = s_wave[w];
                if (w < wave) before += v;
                total += v;
            }
            const int pos = done + before + __popcll(mask & ((1ull << lane) - 1ull));
            if (flag && pos < capc) {
                const float4 raw = *reinterpret_cast<const float4*>(boxes + (size_t)i * 4);
                cbox[pos] = norm_box(raw.x, raw.y, raw.z, raw.w);
                cscore[pos] = s;
                cidx[pos] = i;
            }
            done += total;
            __syncthreads();                                                    // s_wave is rewritten by the next pass; the last one publishes the entries
        }
    }
    if (done == 0) {                                                            // no live row (or nothing to pick)
        if (tid == 0) a.out_cnt[b] = 0;
        return;
    }
    if (done <= capc) {
        soft_pick_loop<false>(a, b, mo, done, cscore, cidx, cbox, boxes, s_best);
    } else {
        float* fscore = reinterpret_cast<float*>(soft_lds);                     // [n], over the compacted rows (every thread is past their last barrier)
        for (int i = tid; i < n_eff; i += SOFT_THREADS) {                       // the owner fills its own entries
            float s;
            fscore[i] = live(i, s) ? s : -INFINITY;
        }
        soft_pick_loop<true>(a, b, mo, n_eff, fscore, nullptr, nullptr, boxes, s_best);
    }
}

// the scores of odtk_detection_pack's rows from the soft-NMS table: one wave per (image, class), the row order of pack_rows_kernel
__global__ void __launch_bounds__(64) pack_scores_kernel(const int* __restrict__ nms_cnt, const float* __restrict__ nms_score, int nc, int cap,
                                                         const int* __restrict__ offsets, float* __restrict__ scores) {
    const int p = blockIdx.x, n = p / nc, c = p % nc, lane = threadIdx.x;
    const int cnt = nms_cnt[p];
    int base = offsets[n];
    for (int k = 0; k < c; ++k) base += nms_cnt[n * nc + k];
    for (int j = lane; j < cnt; j += 64) scores[base + j] = nms_score[(size_t)p * cap + j];
}

}  // namespace
}  // namespace odtk

using namespace odtk;

extern "C" int odtk_soft_nms_image_class(const float* boxes, long long box_istride, const float* scores, long long score_istride, long long score_cstride,
                                         int score_estride, const unsigned char* valid, long long valid_istride, long long valid_cstride, int valid_estride,
                                         int valid_value, int n, const int* n_dev, int N, int num_classes, int max_out, int method, float iou_threshold,
                                         float sigma, float min_score, int* out_idx, float* out_score, int cap, int* out_cnt, void* stream) {
    ODTK_REQUIRE(boxes && scores && out_idx && out_score && out_cnt, "soft_nms_image_class: null pointer");
    ODTK_REQUIRE(method >= 0 && method <= 2, "soft_nms_image_class: method=%d unknown (0 hard, 1 linear, 2 gaussian)", method);
    ODTK_REQUIRE(method != 2 || sigma > 0.f, "soft_nms_image_class: sigma=%g must be positive for the Gaussian method", (double)sigma);
    ODTK_REQUIRE(n > 0 && n <= 32768, "soft_nms_image_class: n=%d out of range (1..32768)", n);
    ODTK_REQUIRE(N > 0 && num_classes > 0 && cap > 0 && (long long)N * num_classes <= 65535, "soft_nms_image_class: N=%d num_classes=%d cap=%d out of range", N,
                 num_classes, cap);
    ODTK_REQUIRE(((uintptr_t)boxes % 16) == 0 && (box_istride % 4) == 0, "soft_nms_image_class: boxes must be 16-byte aligned");
    SoftArgs a;
    a.boxes = boxes; a.box_istride = box_istride;
    a.scores = scores; a.score_istride = score_istride; a.score_cstride = score_cstride; a.score_estride = score_estride;
    a.valid = valid; a.valid_istride = valid_istride; a.valid_cstride = valid_cstride; a.valid_estride = valid_estride; a.valid_value = valid_value;
    a.n = n; a.n_dev = n_dev; a.nc = num_classes;
    a.max_out = max_out; a.method = method;
    a.thr = iou_threshold; a.sigma = sigma; a.min_score = min_score;
    a.out_idx = out_idx; a.out_score = out_score; a.cap = cap; a.out_cnt = out_cnt;
    const size_t lds = n <= SOFT_CAP ? (size_t)n * 24 : ((size_t)n * 4 > (size_t)SOFT_CAP * 24 ? (size_t)n * 4 : (size_t)SOFT_CAP * 24);
    static bool attr_set = false;
    if (!attr_set) {
        ODTK_CHECK_HIP(hipFuncSetAttribute((const void*)soft_nms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4));
        attr_set = true;
    }
    hipLaunchKernelGGL(soft_nms_kernel, dim3(N * num_classes), dim3(SOFT_THREADS), lds, (hipStream_t)stream, a);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}

extern "C" int odtk_detection_pack_scored(const int* nms_idx, const int* nms_cnt, const float* nms_score, int N, int num_classes, int cap, const float* conf,
                                          long long conf_istride, int ldc, const float* boxes, long long box_istride, int* counts, int* offsets,
                                          float* scores, float* bbox, int* class_id, void* stream) {
    ODTK_REQUIRE(nms_idx && nms_cnt && nms_score && conf && boxes && counts && offsets && scores && bbox && class_id, "detection_pack_scored: null pointer");
    // counts, offsets, boxes and class ids: the pack itself (it checks the shapes); then the scores of the same rows from the table
    if (int e = odtk_detection_pack(nms_idx, nms_cnt, N, num_classes, cap, conf, conf_istride, ldc, boxes, box_istride, counts, offsets, scores, bbox,
                                    class_id, stream))
        return e;
    hipLaunchKernelGGL(pack_scores_kernel, dim3(N * num_classes), dim3(64), 0, (hipStream_t)stream, nms_cnt, nms_score, num_classes, cap, offsets, scores);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}
