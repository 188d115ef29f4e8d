// Rows of more than 32 logits (up to wr::MAXC = 256) for the softmax kernels of boxes.hip and retina.hip.
//
// The narrow kernels give a row to one thread and keep it in `float e[32]`; that array cannot grow (at 256 it is the whole register file) and must not be
// indexed by a run-time value (it would live in scratch memory).  Here a row belongs to a GROUP of wr::L = 16 adjacent lanes of one wave (four rows per
// wave): lane j holds the classes c = j + 16 k, k = 0 .. K-1, in K registers, K = 4 / 8 / 16 picked on the host from C (ODTK_WIDE_SLOTS).  Every loop over k has a
// compile-time trip count and is fully unrolled, so v[] stays in registers; a group's 16 lanes read 64 contiguous bytes per k.
//
// Numerics (include/odtk.h states them per entry point):
//   * row maximum: exact (fmaxf over the lane's classes, then a __shfl_xor butterfly over the group);
//   * sum of exponentials: lane j adds ITS classes in ascending order, then the butterfly adds the 16 lane sums with offsets 8, 4, 2, 1.  Float addition is
//     commutative, so all 16 lanes end with the same bits and the result does not depend on anything but the row;
//   * arg-max: the lane's first maximum, then a butterfly on (value, index) in which an equal value with a lower index wins: the lowest index overall.
// Every lane of a wave must reach every shuffle: callers run whole waves through these functions and switch rows off with `on` instead of branching.
#pragma once
#include <math.h>

namespace odtk {
namespace wr {

constexpr int L = 16;          // lanes per row
constexpr int MAXC = 256;      // logits per row, at most

// Host dispatch: runs the statement with K, a compile-time constant, bound to the registers per lane that C logits need (4, 8 or 16)
#define ODTK_WIDE_SLOTS(C, K, ...)                                                                   \
    do {                                                                                             \
        if ((C) <= 4 * odtk::wr::L) { constexpr int K = 4; __VA_ARGS__; }                            \
        else if ((C) <= 8 * odtk::wr::L) { constexpr int K = 8; __VA_ARGS__; }                       \
        else { constexpr int K = 16; __VA_ARGS__; }                                                  \
    } while (0)

__device__ __forceinline__ float group_max(float m) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

__device__ __forceinline__ float group_sum(float s) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// (best, arg) of the group; ties to the lower index
__device__ __forceinline__ void group_argmax(float& best, int& arg) {
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) {
        const float pb = __shfl_xor(best, o);
        const int pa = __shfl_xor(arg, o);
        if (pb > best || (pb == best && pa < arg)) { best = pb; arg = pa; }
    }
}

// lane j's classes of the row z[0 .. C-1]; -inf where the class does not exist or the row is switched off (nothing is read then)
template <int K>
__device__ __forceinline__ void load(const float* z, int C, int j, bool on, float (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = j + L * k;
        v[k] = (on && c < C) ? z[c] : -INFINITY;
    }
}

// v[k] <- exp(v[k] - m) (0 where the class does not exist); m = the row's maximum, s = the sum of the exponentials, the same bits in all 16 lanes
template <int K>
__device__ __forceinline__ void softmax(float (&v)[K], int C, int j, bool on, float& m, float& s) {
    m = v[0];
#pragma unroll
    for (int k = 1; k < K; ++k) m = fmaxf(m, v[k]);
    m = group_max(m);
    s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = (on && j + L * k < C) ? expf(v[k] - m) : 0.f;
        s += v[k];
    }
    s = group_sum(s);
}

}  // namespace wr
}  // namespace odtk
