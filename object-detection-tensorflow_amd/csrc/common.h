// Shared host/device helpers for libodtk (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/odtk.h"

namespace odtk {

void set_error(const char* fmt, ...);
void set_nms_legacy(bool on);   // boxes.hip: odtk_debug_set key 3
void set_gn_small_rows(int rows);   // elementwise.hip: odtk_debug_set key 7
void set_bn_small_rows(int rows); // elementwise.hip: odtk_debug_set key 4 (single-workgroup batch-norm up to this many rows; 0 = off)

#define ODTK_CHECK_HIP(expr)                                                         \
    do {                                                                             \
        hipError_t _e = (expr);                                                      \
        if (_e != hipSuccess) {                                                      \
            odtk::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,            \
                            hipGetErrorString(_e));                                  \
            return ODTK_ERR_HIP;                                                     \
        }                                                                            \
    } while (0)

#define ODTK_REQUIRE(cond, ...)                                                      \
    do {                                                                             \
        if (!(cond)) {                                                               \
            odtk::set_error(__VA_ARGS__);                                            \
            return ODTK_ERR_ARG;                                                     \
        }                                                                            \
    } while (0)

#define ODTK_LAUNCH_CHECK() ODTK_CHECK_HIP(hipGetLastError())

typedef unsigned short bf16_t;   // raw bfloat16 bits

__host__ __device__ inline float bf16_to_f32(bf16_t v) {
    union { uint32_t u; float f; } c;
    c.u = ((uint32_t)v) << 16;
    return c.f;
}
// round-to-nearest-even; NaN kept quiet
__host__ __device__ inline bf16_t f32_to_bf16(float f) {
    union { uint32_t u; float f; } c;
    c.f = f;
    uint32_t u = c.u;
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}

template <typename T> struct elem;
template <> struct elem<bf16_t> {
    __host__ __device__ static float load(bf16_t v) { return bf16_to_f32(v); }
    __host__ __device__ static bf16_t store(float f) { return f32_to_bf16(f); }
};
template <> struct elem<float> {
    __host__ __device__ static float load(float v) { return v; }
    __host__ __device__ static float store(float f) { return f; }
};

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline size_t dtype_size(int dt) { return dt == ODTK_F32 ? 4 : 2; }

// Stream-ordered zero fill by a kernel of this library.  hipMemsetAsync is NOT used inside entry points: captured
// into a HIP graph (ROCm 7.2) its memset node was observed to replay with a garbage fill value (the SSD300 step's
// d(pred) came back as 0x48600000 / 0x70200000 patterns, depending on the host heap layout), api.hip.
int zero_async(void* p, size_t bytes, hipStream_t st);

// boxes.hip: the NMS and decode launches behind the batched inference tail (csrc/detect_batched.hip)
int nms_image_class_launch(const float* boxes, long long box_istride, const float* scores, long long score_istride, long long score_cstride, int score_estride,
                           const unsigned char* valid, long long valid_istride, long long valid_cstride, int valid_estride, int valid_value, int n, const int* n_dev,
                           int N, int nc, int max_out, float iou_threshold, int* out_idx, int cap, int* out_cnt, void* stream);
int decode_launch(const float* pred, long long pred_istride, int N, int A, int C, int ld, const float* box, long long box_istride, int ldb, const float* yx,
                  const float* hw, float score_thr, float* conf, float* boxes, unsigned char* keep, unsigned char* cand, void* stream);

// dense_heads.hip / refinedet.hip: the single-image decodes with an image index (N images per launch; image i's operands px_istride pixels / row_istride rows
// behind those of image i - 1, 0 with N = 1; outputs and the CenterNet workspace packed per image) -- behind odtk_centernet_decode / odtk_refinedet_decode
// and their batched forms (csrc/detect_batched.hip).  The callers check the pointers and N, the launchers the shapes.
int centernet_decode_launch(const float* keypoints, const float* offset, const float* size, long long px_istride, int N, int H, int W, int C, float stride,
                            float score_threshold, int top_k, float* scores, float* bbox, int* class_id, int* count, void* workspace, void* stream);
int refinedet_decode_launch(const float* arm_loc, const float* arm_conf, const float* odm_loc, const float* odm_conf, long long row_istride, int N, int A,
                            int C, const float* yx, const float* hw, float score_threshold, float* conf, float* boxes, unsigned char* keep,
                            unsigned char* cand, void* stream);

}  // namespace odtk
