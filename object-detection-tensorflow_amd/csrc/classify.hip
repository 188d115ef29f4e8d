// Held-out classification metrics over the logits of the pre-training head: per-row rank of the label and cross-entropy, then top-1 / top-k hits, the loss
// sum and per-class counts ACCUMULATED into the caller's buffers (zeroed once per evaluation).  Contract in include/odtk.h ("Classification metrics"),
// restated in NumPy float64 by tests/classify_cases.py.  No counterpart in the reference, which reports the training batch's own accuracy only.
//
// Two launches, the dependency between them a launch boundary; no float atomics, no global atomics at all: every output is bit-identical from run to run.
//   rows        one workgroup per row.  Thread t owns columns t, t + 256, ... (at most 4, kept in registers): it counts the logits that rank in front of the
//               label's (greater, or equal at a lower index) and takes the maximum; both go through a 64-lane butterfly, then the four waves in wave order.
//               The sum of exponentials follows the same way.  The arithmetic of the loss (shift by the maximum, ascending columns per thread, butterfly,
//               waves in order, logf(sum) - (logit[label] - max)) is that of gap_softmax_ce_fwd_kernel (csrc/retina.hip): on the same logits the same bits.
//   accumulate  ONE workgroup.  Chunks of 256 rows are staged in LDS; thread 0 adds the chunk's losses to the double in row order while the per-class
//               counts go through an LDS histogram (integer atomics) and the four totals through integer butterflies.  A single workgroup owns the
//               accumulators, so they are updated with plain loads and stores.
// Plain HIP only (barriers, shuffles): the file also runs under the fiber emulation of tests/hip_cpu.
#include "common.h"
#include <math.h>

namespace odtk {
namespace {

constexpr int CE_THREADS = 256, CE_WAVES = CE_THREADS / 64, CE_MAXC = 1024, CE_MAXN = 65535;
constexpr int CE_PER_THREAD = CE_MAXC / CE_THREADS;

__device__ __forceinline__ bool ce_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(CE_THREADS) classify_rows_kernel(const float* __restrict__ logits, int ldl, int C, const int* __restrict__ labels,
                                                                   int* __restrict__ rank, float* __restrict__ loss) {
    __shared__ float s_v[CE_WAVES];
    __shared__ int s_i[CE_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lab = labels[n];
    if (lab < 0 || lab >= C) {                                         // (uniform over the workgroup: nobody is left waiting at a shuffle)
        if (tid == 0) { rank[n] = -1; loss[n] = NAN; }
        return;
    }
    const float* row = logits + (size_t)n * ldl;
    const float zl = row[lab];
    float z[CE_PER_THREAD];
    float m = -INFINITY;
    int ahead = 0;
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k) {
        const int c = tid + k * CE_THREADS;
        if (c < C) {                                                   // pad columns [C, ldl) are never read
            z[k] = row[c];
            ahead += (z[k] > zl || (z[k] == zl && c < lab)) ? 1 : 0;   // NaN compares false on both sides
            if (z[k] > m) m = z[k];
        } else {
            z[k] = 0.f;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o);
        ahead += __shfl_xor(ahead, o);
        if (m2 > m) m = m2;
    }
    if (lane == 0) { s_v[wave] = m; s_i[wave] = ahead; }
    __syncthreads();
    float bm = s_v[0];
    int r = s_i[0];
    for (int w = 1; w < CE_WAVES; ++w) {
        if (s_v[w] > bm) bm = s_v[w];
        r += s_i[w];
    }
    __syncthreads();
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < CE_PER_THREAD; ++k)
        if (tid + k * CE_THREADS < C) e += expf(z[k] - bm);
    for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o);
    if (lane == 0) s_v[wave] = e;
    __syncthreads();
    if (tid == 0) {
        float se = s_v[0];
        for (int w = 1; w < CE_WAVES; ++w) se += s_v[w];
        rank[n] = ce_finite(zl) ? r : C;                               // a label logit that is NaN or +-inf is a miss
        loss[n] = logf(se) - (zl - bm);
    }
}

__global__ void __launch_bounds__(CE_THREADS) classify_accumulate_kernel(int N, int C, const int* __restrict__ labels, int top_k,
                                                                         const int* __restrict__ rank, const float* __restrict__ loss,
                                                                         long long* __restrict__ totals, double* __restrict__ loss_sum,
                                                                         int* __restrict__ class_seen, int* __restrict__ class_hit) {
    __shared__ int s_seen[CE_MAXC], s_hit[CE_MAXC];
    __shared__ float s_loss[CE_THREADS];
    __shared__ int s_rank[CE_THREADS];
    __shared__ int s_tot[CE_WAVES][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int c = tid; c < C; c += CE_THREADS) { s_seen[c] = 0; s_hit[c] = 0; }
    int cnt[4] = {0, 0, 0, 0};                                         // rows counted, top-1 hits, top-k hits, labels outside [0, C)
    double acc = 0.0;
    if (tid == 0) acc = loss_sum[0];
    __syncthreads();
    for (int base = 0; base < N; base += CE_THREADS) {
        const int i = base + tid;
        const int r = i < N ? rank[i] : -2;
        s_rank[tid] = r;
        s_loss[tid] = i < N ? loss[i] : 0.f;
        if (r >= 0) {                                                  // rank >= 0 only where the label is inside [0, C)
            const int lab = labels[i];
            atomicAdd(&s_seen[lab], 1);
            if (r == 0) atomicAdd(&s_hit[lab], 1);
            cnt[0] += 1;
            cnt[1] += r == 0 ? 1 : 0;
            cnt[2] += r < top_k ? 1 : 0;
        } else if (r == -1) {
            cnt[3] += 1;
        }
        __syncthreads();
        if (tid == 0) {
            const int rows = N - base < CE_THREADS ? N - base : CE_THREADS;
            for (int k = 0; k < rows; ++k)
                if (s_rank[k] >= 0) acc += (double)s_loss[k];         // row order
        }
        __syncthreads();
    }
    for (int q = 0; q < 4; ++q) {
        int v = cnt[q];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) s_tot[wave][q] = v;
    }
    __syncthreads();
    if (tid == 0) {
        for (int q = 0; q < 4; ++q) {
            long long v = 0;
            for (int w = 0; w < CE_WAVES; ++w) v += s_tot[w][q];
            totals[q] += v;
        }
        loss_sum[0] = acc;
    }
    for (int c = tid; c < C; c += CE_THREADS) {
        if (s_seen[c]) class_seen[c] += s_seen[c];
        if (s_hit[c]) class_hit[c] += s_hit[c];
    }
}

}  // namespace
}  // namespace odtk

using namespace odtk;

extern "C" int odtk_classify_eval(const float* logits, int ldl, int N, int C, const int* labels, int top_k, int* rank, float* loss, long long* totals,
                                  double* loss_sum, int* class_seen, int* class_hit, void* stream) {
    ODTK_REQUIRE(C >= 1 && C <= CE_MAXC, "classify_eval: C=%d outside [1, %d]", C, CE_MAXC);
    ODTK_REQUIRE(top_k >= 1 && top_k <= C, "classify_eval: top_k=%d outside [1, C=%d]", top_k, C);
    ODTK_REQUIRE(N >= 1 && N <= CE_MAXN, "classify_eval: N=%d outside [1, %d]", N, CE_MAXN);
    ODTK_REQUIRE(ldl >= C, "classify_eval: ldl=%d is less than C=%d", ldl, C);
    ODTK_REQUIRE(logits && labels && rank && loss && totals && loss_sum && class_seen && class_hit, "classify_eval: null pointer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(classify_rows_kernel, dim3(N), dim3(CE_THREADS), 0, st, logits, ldl, C, labels, rank, loss);
    hipLaunchKernelGGL(classify_accumulate_kernel, dim3(1), dim3(CE_THREADS), 0, st, N, C, labels, top_k, rank, loss, totals, loss_sum, class_seen,
                       class_hit);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}
