// Batched inference tail: decode of N images in one launch, NMS over N x num_classes problems, order-preserving row compaction for heads with more rows
// than the NMS takes per problem, and the detection pack (per-image counts -> exclusive scan -> scores / bbox / class_id in the reference's concat order).
// The decode and NMS launches are the kernels of boxes.hip (decode_launch / nms_image_class_launch): per image they compute what odtk_ssd_decode /
// odtk_retina_decode / odtk_nms_batched compute on that image alone, bit for bit.  No float atomics anywhere: two runs give identical bytes.
// CenterNet (peak test + top-k, no NMS) and RefineDet / PFPNetR (two-stage decode, then the tail above) come in the same way: centernet_decode_launch of
// dense_heads.hip and refinedet_decode_launch of refinedet.hip with N images.
#include "common.h"
#include "wide_row.h"

namespace odtk {
namespace {

constexpr int COMPACT_THREADS = 1024;

// One workgroup per image walks its A rows in order, 1024 at a time: flag = the row is a candidate for at least one class; the wave's ballot gives the rank
// inside the wave, the 16 wave counts (LDS) the rank inside the pass, a register carries the count of the passes before.  rows[img][rank] = row index for
// rank < cap_rows; counts[img] = the TRUE number of flagged rows (the host compares it with the capacity).
__global__ void __launch_bounds__(COMPACT_THREADS) compact_rows_kernel(const unsigned char* __restrict__ cand, int A, int ld, int nc, int cap_rows,
                                                                      int* __restrict__ rows, int* __restrict__ counts) {
    __shared__ int s_wave[COMPACT_THREADS / 64];
    const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned char* base = cand + (size_t)img * A * ld;
    int* out = rows + (size_t)img * cap_rows;
    const bool words = (nc % 4) == 0 && (ld % 4) == 0 && (reinterpret_cast<uintptr_t>(cand) % 4) == 0;
    int done = 0;
    for (int a0 = 0; a0 < A; a0 += COMPACT_THREADS) {           // (whole workgroups enter: ballots and barriers need every thread)
        const int a = a0 + tid;
        bool flag = false;
        if (a < A) {
            const unsigned char* row = base + (size_t)a * ld;
            if (words) {
                const unsigned* w = reinterpret_cast<const unsigned*>(row);
                unsigned acc = 0u;
                for (int c = 0; c < nc / 4; ++c) acc |= w[c];
                flag = acc != 0u;
            } else {
                for (int c = 0; c < nc; ++c) flag = flag || row[c] != 0;
            }
        }
        const unsigned long long mask = __ballot(flag);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < COMPACT_THREADS / 64; ++w) {
            const int v = s_wave[w];
            if (w < wave) before += v;
            total += v;
        }
        const int pos = done + before + __popcll(mask & ((1ull << lane) - 1ull));
        if (flag && pos < cap_rows) out[pos] = a;
        done += total;
        __syncthreads();                                        // s_wave is rewritten by the next pass
    }
    if (tid == 0) counts[img] = done;
}

// conf / boxes / cand of the compacted rows, [N][cap_rows][nc | 4 | nc]; rows past an image's count are left as they are (the NMS stops at the count)
__global__ void gather_rows_kernel(const int* __restrict__ rows, const int* __restrict__ counts, int A, int cap_rows, int nc, const float* __restrict__ conf,
                                   int ldc, const float* __restrict__ boxes, const unsigned char* __restrict__ cand, int ldk, float* __restrict__ conf_out,
                                   float* __restrict__ boxes_out, unsigned char* __restrict__ cand_out) {
    const int img = blockIdx.y;
    int cnt = counts[img];
    if (cnt > cap_rows) cnt = cap_rows;
    const int* map = rows + (size_t)img * cap_rows;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < (long long)cnt * nc) {
        const int j = (int)(e / nc), c = (int)(e % nc);
        const size_t src = (size_t)img * A + map[j];
        conf_out[((size_t)img * cap_rows + j) * nc + c] = conf[src * ldc + c];
        cand_out[((size_t)img * cap_rows + j) * nc + c] = cand[src * ldk + c];
    }
    if (e < (long long)cnt * 4) {
        const int j = (int)(e / 4), c = (int)(e % 4);
        boxes_out[((size_t)img * cap_rows + j) * 4 + c] = boxes[((size_t)img * A + map[j]) * 4 + c];
    }
}

constexpr int PACK_MAX_IMAGES = 1024;

// counts[n] = sum over classes of nms_cnt[n][c]; offsets[0..N] = their exclusive scan (offsets[N] = K): one workgroup, Hillis-Steele over LDS
__global__ void __launch_bounds__(PACK_MAX_IMAGES) pack_scan_kernel(const int* __restrict__ nms_cnt, int N, int nc, int* __restrict__ counts,
                                                                   int* __restrict__ offsets) {
    __shared__ int s[2][PACK_MAX_IMAGES];
    const int n = threadIdx.x;
    int total = 0;
    if (n < N)
        for (int c = 0; c < nc; ++c) total += nms_cnt[n * nc + c];
    s[0][n] = total;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < PACK_MAX_IMAGES; o <<= 1) {
        s[cur ^ 1][n] = s[cur][n] + (n >= o ? s[cur][n - o] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (n < N) {
        counts[n] = total;
        offsets[n + 1] = s[cur][n];
        if (n == 0) offsets[0] = 0;
    }
}

// one wave per (image, class): its picks go behind those of the image's lower classes, in NMS pick order (the reference's concat order, SSD300.py:172-190)
__global__ void __launch_bounds__(64) pack_rows_kernel(const int* __restrict__ nms_idx, const int* __restrict__ nms_cnt, int nc, int cap,
                                                       const float* __restrict__ conf, long long conf_istride, int ldc, const float* __restrict__ boxes,
                                                       long long box_istride, const int* __restrict__ offsets, float* __restrict__ scores,
                                                       float* __restrict__ bbox, int* __restrict__ class_id) {
    const int p = blockIdx.x, n = p / nc, c = p % nc, lane = threadIdx.x;
    const int cnt = nms_cnt[p];
    int base = offsets[n];
    for (int k = 0; k < c; ++k) base += nms_cnt[n * nc + k];
    const int* ids = nms_idx + (size_t)p * cap;
    const float* cf = conf + (size_t)n * conf_istride;
    const float* bx = boxes + (size_t)n * box_istride;
    for (int j = lane; j < cnt; j += 64) {
        const int id = ids[j];
        scores[base + j] = cf[(size_t)id * ldc + c];
        for (int k = 0; k < 4; ++k) bbox[(size_t)(base + j) * 4 + k] = bx[(size_t)id * 4 + k];
        class_id[base + j] = c;
    }
}

}  // namespace
}  // namespace odtk

using namespace odtk;

extern "C" int odtk_ssd_decode_batched(const float* pred, int N, int A, int C, int ld, const float* yx, const float* hw, float score_thr, float* conf,
                                       float* boxes, unsigned char* keep, unsigned char* cand, void* stream) {
    ODTK_REQUIRE(pred && yx && hw && conf && boxes && keep && cand, "ssd_decode_batched: null pointer");
    ODTK_REQUIRE(C > 1 && C <= wr::MAXC && ld >= C + 4, "ssd_decode_batched: C=%d ld=%d unsupported (2 <= C <= %d, ld >= C + 4)", C, ld, wr::MAXC);
    ODTK_REQUIRE(N > 0 && N <= 65535 && A > 0, "ssd_decode_batched: N=%d A=%d out of range", N, A);
    return decode_launch(pred, (long long)A * ld, N, A, C, ld, pred + C, (long long)A * ld, ld, yx, hw, score_thr, conf, boxes, keep, cand, stream);
}

extern "C" int odtk_retina_decode_batched(const float* pconf, const float* pbox, int N, int A, int C, const float* yx, const float* hw, float score_thr,
                                          float* conf, float* boxes, unsigned char* keep, unsigned char* cand, void* stream) {
    ODTK_REQUIRE(pconf && pbox && yx && hw && conf && boxes && keep && cand, "retina_decode_batched: null pointer");
    ODTK_REQUIRE(C > 1 && C <= wr::MAXC && A > 0, "retina_decode_batched: C=%d A=%d unsupported (2 <= C <= %d)", C, A, wr::MAXC);
    ODTK_REQUIRE(N > 0 && N <= 65535, "retina_decode_batched: N=%d out of range", N);
    return decode_launch(pconf, (long long)A * C, N, A, C, C, pbox, (long long)A * 4, 4, yx, hw, score_thr, conf, boxes, keep, cand, stream);
}

extern "C" int odtk_refinedet_decode_batched(const float* arm_loc, const float* arm_conf, const float* odm_loc, const float* odm_conf, int N, int A, int C,
                                             const float* yx, const float* hw, float score_thr, float* conf, float* boxes, unsigned char* keep,
                                             unsigned char* cand, void* stream) {
    ODTK_REQUIRE(arm_loc && arm_conf && odm_loc && odm_conf && yx && hw && conf && boxes && keep && cand, "refinedet_decode_batched: null pointer");
    ODTK_REQUIRE(N > 0 && N <= 65535, "refinedet_decode_batched: N=%d out of range (1..65535)", N);
    return refinedet_decode_launch(arm_loc, arm_conf, odm_loc, odm_conf, A, N, A, C, yx, hw, score_thr, conf, boxes, keep, cand, stream);
}

// N score planes (f32) + N class planes (i32); odtk_centernet_workspace_bytes (the loss's sizing) holds ONE of each
extern "C" long long odtk_centernet_decode_workspace_bytes(int N, int H, int W) { return (long long)N * H * W * 8; }

extern "C" int odtk_centernet_decode_batched(const float* keypoints, const float* offset, const float* size, int N, int H, int W, int C, float stride,
                                             float score_threshold, int top_k, float* scores, float* bbox, int* class_id, int* counts, void* workspace,
                                             void* stream) {
    ODTK_REQUIRE(keypoints && offset && size && scores && bbox && class_id && counts && workspace, "centernet_decode_batched: null pointer");
    ODTK_REQUIRE(N > 0 && N <= 65535, "centernet_decode_batched: N=%d out of range (1..65535)", N);
    return centernet_decode_launch(keypoints, offset, size, (long long)H * W, N, H, W, C, stride, score_threshold, top_k, scores, bbox, class_id, counts,
                                   workspace, stream);
}

extern "C" int odtk_nms_image_class(const float* boxes, long long box_istride, const float* scores, long long score_istride, long long score_cstride,
                                    int score_estride, const unsigned char* valid, long long valid_istride, long long valid_cstride, int valid_estride,
                                    int valid_value, int n, const int* n_dev, int N, int num_classes, int max_out, float iou_threshold, int* out_idx, int cap,
                                    int* out_cnt, void* stream) {
    ODTK_REQUIRE(boxes && scores && out_idx && out_cnt, "nms_image_class: null pointer");
    ODTK_REQUIRE(n > 0 && n <= 32768, "nms_image_class: n=%d out of range (1..32768)", n);
    ODTK_REQUIRE(N > 0 && num_classes > 0 && cap > 0 && (long long)N * num_classes <= 65535, "nms_image_class: N=%d num_classes=%d cap=%d out of range", N,
                 num_classes, cap);
    ODTK_REQUIRE(((uintptr_t)boxes % 16) == 0 && (box_istride % 4) == 0, "nms_image_class: boxes must be 16-byte aligned");
    return nms_image_class_launch(boxes, box_istride, scores, score_istride, score_cstride, score_estride, valid, valid_istride, valid_cstride, valid_estride,
                                  valid_value, n, n_dev, N, num_classes, max_out, iou_threshold, out_idx, cap, out_cnt, stream);
}

extern "C" int odtk_compact_rows(const unsigned char* cand, int N, int A, int ld, int num_classes, int cap_rows, int* rows, int* counts, void* stream) {
    ODTK_REQUIRE(cand && rows && counts, "compact_rows: null pointer");
    ODTK_REQUIRE(N > 0 && N <= 65535 && A > 0 && num_classes > 0 && ld >= num_classes && cap_rows > 0, "compact_rows: N=%d A=%d ld=%d num_classes=%d cap_rows=%d",
                 N, A, ld, num_classes, cap_rows);
    hipLaunchKernelGGL(compact_rows_kernel, dim3(N), dim3(COMPACT_THREADS), 0, (hipStream_t)stream, cand, A, ld, num_classes, cap_rows, rows, counts);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}

extern "C" int odtk_gather_rows(const int* rows, const int* counts, int N, int A, int cap_rows, int num_classes, const float* conf, int ldc,
                                const float* boxes, const unsigned char* cand, int ldk, float* conf_out, float* boxes_out, unsigned char* cand_out,
                                void* stream) {
    ODTK_REQUIRE(rows && counts && conf && boxes && cand && conf_out && boxes_out && cand_out, "gather_rows: null pointer");
    ODTK_REQUIRE(N > 0 && N <= 65535 && A > 0 && cap_rows > 0 && num_classes > 0 && ldc >= num_classes && ldk >= num_classes,
                 "gather_rows: N=%d A=%d cap_rows=%d num_classes=%d ldc=%d ldk=%d", N, A, cap_rows, num_classes, ldc, ldk);
    const long long per = (long long)cap_rows * (num_classes > 4 ? num_classes : 4);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((per + 255) / 256), N), dim3(256), 0, (hipStream_t)stream, rows, counts, A, cap_rows, num_classes,
                       conf, ldc, boxes, cand, ldk, conf_out, boxes_out, cand_out);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}

extern "C" int odtk_detection_pack(const int* nms_idx, const int* nms_cnt, int N, int num_classes, int cap, const float* conf, long long conf_istride, int ldc,
                                   const float* boxes, long long box_istride, int* counts, int* offsets, float* scores, float* bbox, int* class_id,
                                   void* stream) {
    ODTK_REQUIRE(nms_idx && nms_cnt && conf && boxes && counts && offsets && scores && bbox && class_id, "detection_pack: null pointer");
    ODTK_REQUIRE(N > 0 && N <= PACK_MAX_IMAGES && num_classes > 0 && cap > 0 && ldc >= num_classes && (long long)N * num_classes <= 0x7fffffffLL / cap,
                 "detection_pack: N=%d (max %d) num_classes=%d cap=%d ldc=%d", N, PACK_MAX_IMAGES, num_classes, cap, ldc);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(PACK_MAX_IMAGES), 0, st, nms_cnt, N, num_classes, counts, offsets);
    hipLaunchKernelGGL(pack_rows_kernel, dim3(N * num_classes), dim3(64), 0, st, nms_idx, nms_cnt, num_classes, cap, conf, conf_istride, ldc, boxes,
                       box_istride, offsets, scores, bbox, class_id);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}
