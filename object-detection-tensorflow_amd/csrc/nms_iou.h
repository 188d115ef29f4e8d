// The box normalisation and IoU of the NMS kernels (NonMaxSuppressionV3's IOU()), restated from boxes.hip for csrc/soft_nms.hip: the same expressions in the
// same order, so the `hard` method of odtk_soft_nms_image_class picks what odtk_nms_image_class picks (tests/test_gpu_soft_nms.py holds the two together).
#pragma once
#include "common.h"

namespace odtk {
namespace nms_iou {

struct NBox { float ymin, xmin, ymax, xmax; };

__device__ __forceinline__ NBox norm_box(float b0, float b1, float b2, float b3) {
    NBox r;
    r.ymin = fminf(b0, b2); r.xmin = fminf(b1, b3);
    r.ymax = fmaxf(b0, b2); r.xmax = fmaxf(b1, b3);
    return r;
}
// 0 when either area <= 0
__device__ __forceinline__ float iou_nms(const NBox& a, const NBox& b) {
    const float area_a = (a.ymax - a.ymin) * (a.xmax - a.xmin);
    const float area_b = (b.ymax - b.ymin) * (b.xmax - b.xmin);
    if (area_a <= 0.f || area_b <= 0.f) return 0.f;
    const float iymin = fmaxf(a.ymin, b.ymin), ixmin = fmaxf(a.xmin, b.xmin);
    const float iymax = fminf(a.ymax, b.ymax), ixmax = fminf(a.xmax, b.xmax);
    const float inter = fmaxf(iymax - iymin, 0.f) * fmaxf(ixmax - ixmin, 0.f);
    return inter / (area_a + area_b - inter);
}

}  // namespace nms_iou
}  // namespace odtk
