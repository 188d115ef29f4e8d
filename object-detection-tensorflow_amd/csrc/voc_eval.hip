// PASCAL VOC detection metric (per-class AP, 11-point or area) over a whole validation set, on the device from upload to AP.
// No counterpart in the reference (its val_generator is "not used", testSSD300.py:56-58); the semantics are pinned in include/odtk.h and restated in
// NumPy by tests/voc_eval_ref.py.
//
// Pipeline (every cross-workgroup dependency is a launch boundary; integer atomics only, so every output is bit-identical from run to run):
//   init     tp_out = 0, identity index lists, per-class counts of valid detections (ndet) and GT rows (npos) by LDS histograms
//   sort A   stable LSD radix sort of the detection indices by (class, descending score): 4 passes on the score bits, then 1-2 on the class
//            -> the per-class global rank order (ties keep sequence order because every pass is stable)
//   sort B   the order of A, stable-sorted by image (0-3 passes) -> contiguous (image, class) segments, rank order inside each
//   sort G   GT indices stable-sorted by the (image, class) key -> contiguous GT segments in row order
//   match    one thread per segment head walks its detections in rank order against the segment's GT rows (binary search for the range, a
//            byte per GT row as the "taken" flag -- each GT row belongs to exactly one segment, so one thread owns it) and writes tp_out
//   ap       one workgroup per class walks the rank order of A backwards in chunks: cumulative TP by a block scan, recall / precision in f64,
//            the 11-point maxima or the precision envelope (suffix max) and the area sum (fixed-order tree reduction)
// A radix pass is three launches: per-block digit histograms (+ digit totals by integer atomics), one workgroup per digit scanning its row of
// block counts, and a stable scatter (wave ranks by 8 ballots, waves in order through LDS).
#include "common.h"
#include <float.h>
#include <math.h>

namespace odtk {
namespace {

constexpr int VE_THREADS = 256;
constexpr int VE_ITEMS = 16;                              // elements per thread and radix tile
constexpr int VE_TILE = VE_THREADS * VE_ITEMS;
constexpr int VE_MAX_PASSES = 16;
constexpr int VE_AP_ITEMS = 8;                            // rank positions per thread and AP chunk
constexpr int VE_MAX_DET = 8 << 20, VE_MAX_GT = 2 << 20, VE_MAX_IMAGES = 1 << 20, VE_MAX_CLASSES = 1024;

struct VocIn {
    const float* scores; const float* boxes; const int* det_cls; const int* det_img;
    const float* gt; const int* gt_img;
    int D, G, I, C;
};

__device__ __forceinline__ bool det_valid(const VocIn& a, int i) {
    const unsigned u = __float_as_uint(a.scores[i]);
    const int c = a.det_cls[i], m = a.det_img[i];
    return (u & 0x7f800000u) != 0x7f800000u && c >= 0 && c < a.C && m >= 0 && m < a.I;
}
// class key in [0, C]: C = not a valid detection (sorts behind every class, skipped by match and AP)
__device__ __forceinline__ int det_class_key(const VocIn& a, int i) { return det_valid(a, i) ? a.det_cls[i] : a.C; }
__device__ __forceinline__ int det_image_key(const VocIn& a, int i) { return det_valid(a, i) ? a.det_img[i] : 0; }
__device__ __forceinline__ int det_segment(const VocIn& a, int i) { return det_image_key(a, i) * (a.C + 1) + det_class_key(a, i); }
// descending score -> ascending key (order-preserving f32 bits, inverted; -0 and +0 are one score)
__device__ __forceinline__ unsigned score_key(float s) {
    unsigned u = s == 0.f ? 0u : __float_as_uint(s);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}
__device__ __forceinline__ int gt_class(const VocIn& a, int j) {          // -1 = padding / not counted
    const float c = a.gt[(size_t)j * 5 + 4];
    const int m = a.gt_img[j];
    return (c >= 0.f && c < (float)a.C && m >= 0 && m < a.I) ? (int)c : -1;
}
__device__ __forceinline__ int gt_segment(const VocIn& a, int j) {
    const int c = gt_class(a, j);
    const int m = a.gt_img[j];
    return c >= 0 ? m * (a.C + 1) + c : ((m >= 0 && m < a.I) ? m * (a.C + 1) + a.C : a.C);
}

enum { KEY_SCORE = 0, KEY_CLASS = 1, KEY_IMAGE = 2, KEY_GT = 3 };
__device__ __forceinline__ int radix_digit(const VocIn& a, int mode, int shift, int idx) {
    unsigned k;
    if (mode == KEY_SCORE) k = score_key(a.scores[idx]);
    else if (mode == KEY_CLASS) k = (unsigned)det_class_key(a, idx);
    else if (mode == KEY_IMAGE) k = (unsigned)det_image_key(a, idx);
    else k = (unsigned)gt_segment(a, idx);
    return (int)((k >> shift) & 255u);
}

// ---------------------------------------------------------------- init: outputs, identity lists, per-class counts
__global__ void __launch_bounds__(VE_THREADS) voc_init_kernel(VocIn a, unsigned char* tp_out, int* det_idx, int* gt_idx, unsigned char* taken,
                                                              int* ndet, int* npos) {
    __shared__ int hd[VE_MAX_CLASSES], hg[VE_MAX_CLASSES];
    const int t = threadIdx.x;
    for (int c = t; c < a.C; c += VE_THREADS) { hd[c] = 0; hg[c] = 0; }
    __syncthreads();
    const int base = blockIdx.x * VE_TILE;
    for (int k = 0; k < VE_ITEMS; ++k) {
        const int i = base + k * VE_THREADS + t;
        if (i < a.D) {
            tp_out[i] = 0;
            det_idx[i] = i;
            if (det_valid(a, i)) atomicAdd(&hd[a.det_cls[i]], 1);
        }
        if (i < a.G) {
            gt_idx[i] = i;
            taken[i] = 0;
            const int c = gt_class(a, i);
            if (c >= 0) atomicAdd(&hg[c], 1);
        }
    }
    __syncthreads();
    for (int c = t; c < a.C; c += VE_THREADS) {
        if (hd[c]) atomicAdd(&ndet[c], hd[c]);
        if (hg[c]) atomicAdd(&npos[c], hg[c]);
    }
}

// ---------------------------------------------------------------- one stable LSD radix pass over an index list (8-bit digit)
// hist[d * nb + b]: elements of tile b with digit d (digit-major: its exclusive scan is the scatter base of every (digit, tile)); tot[d] += the same
__global__ void __launch_bounds__(VE_THREADS) voc_radix_hist_kernel(VocIn a, int mode, int shift, const int* in, int n, int nb, unsigned* hist,
                                                                    unsigned* tot) {
    __shared__ unsigned h[256];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const int base = blockIdx.x * VE_TILE;
    for (int k = 0; k < VE_ITEMS; ++k) {
        const int i = base + k * VE_THREADS + t;
        if (i < n) atomicAdd(&h[radix_digit(a, mode, shift, in[i])], 1u);
    }
    __syncthreads();
    hist[(size_t)t * nb + blockIdx.x] = h[t];
    if (h[t]) atomicAdd(&tot[t], h[t]);
}

template <typename T, typename Op>
__device__ __forceinline__ T block_incl_scan(T v, T* sh, Op op) {             // 256 threads, Hillis-Steele in LDS
    const int t = threadIdx.x;
    for (int off = 1; off < VE_THREADS; off <<= 1) {
        sh[t] = v;
        __syncthreads();
        if (t >= off) v = op(sh[t - off], v);
        __syncthreads();
    }
    return v;
}
struct AddU { __device__ unsigned operator()(unsigned x, unsigned y) const { return x + y; } };
struct AddI { __device__ int operator()(int x, int y) const { return x + y; } };
struct MaxD { __device__ double operator()(double x, double y) const { return x > y ? x : y; } };

// one workgroup per digit d: exclusive scan of row d of hist, offset by the counts of all smaller digits
__global__ void __launch_bounds__(VE_THREADS) voc_radix_scan_kernel(unsigned* hist, int nb, const unsigned* tot) {
    __shared__ unsigned sh[VE_THREADS];
    const int d = blockIdx.x, t = threadIdx.x;
    const unsigned before = block_incl_scan((t < d) ? tot[t] : 0u, sh, AddU());
    if (t == VE_THREADS - 1) sh[0] = before;
    __syncthreads();
    unsigned carry = sh[0];
    __syncthreads();
    unsigned* row = hist + (size_t)d * nb;
    for (int s = 0; s < nb; s += VE_THREADS) {
        const unsigned v = s + t < nb ? row[s + t] : 0u;
        const unsigned incl = block_incl_scan(v, sh, AddU());
        if (s + t < nb) row[s + t] = carry + incl - v;
        if (t == VE_THREADS - 1) sh[0] = incl;
        __syncthreads();
        carry += sh[0];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(VE_THREADS) voc_radix_scatter_kernel(VocIn a, int mode, int shift, const int* in, int* out, int n, int nb,
                                                                       const unsigned* hist) {
    __shared__ unsigned base[256];
    __shared__ unsigned wcnt[VE_THREADS / 64][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    base[t] = hist[(size_t)t * nb + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < VE_ITEMS; ++k) {
        const int i = blockIdx.x * VE_TILE + k * VE_THREADS + t;
        const bool ok = i < n;
        const int v = ok ? in[i] : 0;
        const int d = ok ? radix_digit(a, mode, shift, v) : 0;
        for (int w = 0; w < VE_THREADS / 64; ++w) wcnt[w][t] = 0;
        unsigned long long peers = __ballot(ok);
        for (int bit = 0; bit < 8; ++bit) {
            const unsigned long long m = __ballot((d >> bit) & 1);
            peers &= ((d >> bit) & 1) ? m : ~m;
        }
        const int rank = __popcll(peers & below);
        __syncthreads();
        if (ok && rank == 0) wcnt[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        unsigned run = base[t];
        for (int w = 0; w < VE_THREADS / 64; ++w) {
            const unsigned c = wcnt[w][t];
            wcnt[w][t] = run;
            run += c;
        }
        base[t] = run;
        __syncthreads();
        if (ok) out[wcnt[wave][d] + rank] = v;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- greedy match per (image, class) segment
__device__ __forceinline__ int gt_lower_bound(const VocIn& a, const int* gidx, int key) {
    int lo = 0, hi = a.G;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (gt_segment(a, gidx[mid]) < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(VE_THREADS) voc_match_kernel(VocIn a, const int* order, const int* gidx, unsigned char* taken, float iou_thr,
                                                               unsigned char* tp_out) {
    const int p = blockIdx.x * VE_THREADS + threadIdx.x;
    if (p >= a.D) return;
    const int seg = det_segment(a, order[p]);
    if (p > 0 && det_segment(a, order[p - 1]) == seg) return;              // not the head of its segment
    if (seg % (a.C + 1) == a.C) return;                                    // invalid detections
    const int g0 = gt_lower_bound(a, gidx, seg), g1 = gt_lower_bound(a, gidx, seg + 1);
    for (int q = p; q < a.D; ++q) {
        const int i = order[q];
        if (q > p && det_segment(a, i) != seg) break;
        const float y1d = a.boxes[(size_t)i * 4 + 0], x1d = a.boxes[(size_t)i * 4 + 1];
        const float y2d = a.boxes[(size_t)i * 4 + 2], x2d = a.boxes[(size_t)i * 4 + 3];
        const float ad = (y2d - y1d) * (x2d - x1d);
        float best = -1.f;
        int bj = -1;
        for (int m = g0; m < g1; ++m) {
            const float* r = a.gt + (size_t)gidx[m] * 5;
            const float yc = r[0], xc = r[1], h = r[2], w = r[3];
            const float y1g = yc - h / 2.f, x1g = xc - w / 2.f, y2g = yc + h / 2.f, x2g = xc + w / 2.f;
            const float ih = fmaxf(fminf(y2d, y2g) - fmaxf(y1d, y1g), 0.f);
            const float iw = fmaxf(fminf(x2d, x2g) - fmaxf(x1d, x1g), 0.f);
            const float inter = ih * iw;
            const float uni = ad + (y2g - y1g) * (x2g - x1g) - inter;
            const float iou = uni > 0.f ? inter / uni : 0.f;
            if (iou > best) { best = iou; bj = m; }
        }
        if (bj >= 0 && best > iou_thr && !taken[bj]) {
            taken[bj] = 1;
            tp_out[i] = 1;
        }
    }
}

// ---------------------------------------------------------------- AP per class
__global__ void __launch_bounds__(VE_THREADS) voc_ap_kernel(VocIn a, const int* order, const int* ndet, const int* npos, const unsigned char* tp,
                                                            int metric, double* ap_out) {
    __shared__ int shi[VE_THREADS];
    __shared__ double shd[VE_THREADS];
    __shared__ double pk_sh[11][VE_THREADS];
    const int c = blockIdx.x, t = threadIdx.x;
    int before = 0;
    for (int k = t; k < c; k += VE_THREADS) before += ndet[k];
    before = block_incl_scan(before, shi, AddI());
    if (t == VE_THREADS - 1) shi[0] = before;
    __syncthreads();
    const int start = shi[0], n = ndet[c], np = npos[c];
    __syncthreads();
    if (np == 0) {                                                          // no GT: undefined, left out of the mean
        if (t == 0) ap_out[c] = __builtin_nan("");
        return;
    }
    // total TP of the class
    int mine = 0;
    for (int k = t; k < n; k += VE_THREADS) mine += tp[order[start + k]];
    mine = block_incl_scan(mine, shi, AddI());
    if (t == VE_THREADS - 1) shi[0] = mine;
    __syncthreads();
    const int total = shi[0];
    __syncthreads();
    const double dn = (double)np;
    double thr[11], pk[11];
    for (int k = 0; k < 11; ++k) { thr[k] = (double)k * 0.1; pk[k] = -1.0; }   // t_k = k * 0.1 in double: np.arange(0., 1.1, 0.1)
    int after_carry = 0;                                                    // TP at rank positions behind the current chunk
    double env_carry = 0.0;                                                 // max precision behind the current chunk (the sentinel 0 included)
    double area = 0.0;
    const int CH = VE_THREADS * VE_AP_ITEMS;
    for (int end = n; end > 0; end -= CH) {                                 // chunks from the back: [end - CH, end)
        const int s = end - CH;
        const int p0 = s + t * VE_AP_ITEMS;
        int f[VE_AP_ITEMS];
        int cnt = 0;
        for (int j = 0; j < VE_AP_ITEMS; ++j) {
            const int k = p0 + j;
            f[j] = (k >= 0 && k < end) ? tp[order[start + k]] : 0;
            cnt += f[j];
        }
        // TP behind this thread's items: a suffix scan = a prefix scan over reversed threads
        const int incl = block_incl_scan(cnt, shi, AddI());                // (prefix over t; the suffix is chunk total - incl)
        if (t == VE_THREADS - 1) shi[0] = incl;
        __syncthreads();
        const int chunk_tp = shi[0];
        __syncthreads();
        int after = after_carry + chunk_tp - incl;
        double prec[VE_AP_ITEMS];
        int tpc[VE_AP_ITEMS];
        double lmax = 0.0;
        for (int j = VE_AP_ITEMS - 1; j >= 0; --j) {
            const int k = p0 + j;
            if (k >= 0 && k < end) {
                after += f[j];
                tpc[j] = total - after + f[j];                              // cumulative TP up to and including position k
                prec[j] = (double)tpc[j] / fmax((double)(k + 1), DBL_EPSILON);
                const double rec = (double)tpc[j] / dn;
                if (prec[j] > lmax) lmax = prec[j];
                for (int q = 0; q < 11; ++q)
                    if (rec >= thr[q] && prec[j] > pk[q]) pk[q] = prec[j];
            } else {
                tpc[j] = 0;
                prec[j] = 0.0;
            }
        }
        // precision envelope: max over this thread's later items, the later threads of the chunk and the chunk behind
        shd[VE_THREADS - 1 - t] = lmax;                                     // suffix max = prefix max over the reversed threads
        __syncthreads();
        double sv = shd[t];
        __syncthreads();
        sv = block_incl_scan(sv, shd, MaxD());
        shd[VE_THREADS - 1 - t] = sv;                                       // shd[t] = max over threads >= t
        __syncthreads();
        double env = fmax(env_carry, t + 1 < VE_THREADS ? shd[t + 1] : 0.0);
        const double chunk_max = shd[0];
        __syncthreads();
        for (int j = VE_AP_ITEMS - 1; j >= 0; --j) {
            const int k = p0 + j;
            if (k < 0 || k >= end) continue;
            env = fmax(env, prec[j]);
            if (f[j]) area += ((double)tpc[j] / dn - (double)(tpc[j] - 1) / dn) * env;
        }
        after_carry += chunk_tp;
        env_carry = fmax(env_carry, chunk_max);
    }
    double r;
    if (metric == 0) {
        for (int q = 0; q < 11; ++q) pk_sh[q][t] = pk[q];
        __syncthreads();
        if (t == 0) {
            r = 0.0;
            for (int q = 0; q < 11; ++q) {
                double m = -1.0;
                for (int u = 0; u < VE_THREADS; ++u) m = fmax(m, pk_sh[q][u]);
                r += (m < 0.0 ? 0.0 : m) / 11.0;
            }
            ap_out[c] = r;
        }
    } else {
        shd[t] = area;                                                      // fixed-order tree sum
        __syncthreads();
        for (int off = VE_THREADS / 2; off > 0; off >>= 1) {
            if (t < off) shd[t] = shd[t] + shd[t + off];
            __syncthreads();
        }
        if (t == 0) ap_out[c] = shd[0];
    }
}

int bits_for(long long maxval) {                                           // bits to represent 0..maxval
    int b = 0;
    while (b < 62 && (1ll << b) <= maxval) ++b;
    return b;
}
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct VocLayout {
    size_t idx[3], gidx[2], taken, hist, tot, ndet, total;
    int nb;
};
VocLayout voc_layout(int D, int G, int C) {
    VocLayout L;
    const long long nmax = D > G ? D : G;
    L.nb = (int)((nmax + VE_TILE - 1) / VE_TILE);
    if (L.nb < 1) L.nb = 1;
    size_t off = 0;
    for (int k = 0; k < 3; ++k) { L.idx[k] = off; off += align256((size_t)D * 4); }
    for (int k = 0; k < 2; ++k) { L.gidx[k] = off; off += align256((size_t)G * 4); }
    L.taken = off; off += align256((size_t)G);
    L.hist = off; off += align256((size_t)256 * L.nb * 4);
    L.tot = off; off += align256((size_t)256 * VE_MAX_PASSES * 4);
    L.ndet = off; off += align256((size_t)(C + 1) * 4);
    L.total = off;
    return L;
}

bool voc_sizes_ok(int D, int G, int I, int C) {
    return D >= 0 && D <= VE_MAX_DET && G >= 0 && G <= VE_MAX_GT && I >= 1 && I <= VE_MAX_IMAGES && C >= 1 && C <= VE_MAX_CLASSES;
}
#define VOC_SIZES_MSG "voc_eval: num_det=%d num_gt=%d num_images=%d num_classes=%d outside the supported range (num_det <= %d, num_gt <= %d, " \
                      "1 <= num_images <= %d, 1 <= num_classes <= %d)"

}  // namespace
}  // namespace odtk

using namespace odtk;

extern "C" long long odtk_voc_eval_workspace_bytes(int num_det, int num_gt, int num_images, int num_classes) {
    if (!voc_sizes_ok(num_det, num_gt, num_images, num_classes)) {
        set_error(VOC_SIZES_MSG, num_det, num_gt, num_images, num_classes, VE_MAX_DET, VE_MAX_GT, VE_MAX_IMAGES, VE_MAX_CLASSES);
        return -1;
    }
    return (long long)voc_layout(num_det, num_gt, num_classes).total;
}

extern "C" int odtk_voc_eval(const float* scores, const float* boxes, const int* det_cls, const int* det_img, int num_det, const float* gt_rows,
                             const int* gt_img, int num_gt, int num_images, int num_classes, float iou_thr, int metric, void* workspace,
                             unsigned char* tp_out, int* npos_out, double* ap_out, void* stream) {
    ODTK_REQUIRE(voc_sizes_ok(num_det, num_gt, num_images, num_classes), VOC_SIZES_MSG, num_det, num_gt, num_images, num_classes, VE_MAX_DET,
                 VE_MAX_GT, VE_MAX_IMAGES, VE_MAX_CLASSES);
    ODTK_REQUIRE(metric == 0 || metric == 1, "voc_eval: metric %d (0 = voc07 11-point, 1 = area)", metric);
    ODTK_REQUIRE(workspace && npos_out && ap_out, "voc_eval: null pointer");
    ODTK_REQUIRE(num_det == 0 || (scores && boxes && det_cls && det_img && tp_out), "voc_eval: null detection pointer");
    ODTK_REQUIRE(num_gt == 0 || (gt_rows && gt_img), "voc_eval: null ground-truth pointer");
    const int D = num_det, G = num_gt, I = num_images, C = num_classes;
    const VocLayout L = voc_layout(D, G, C);
    char* ws = (char*)workspace;
    int* idx[3] = {(int*)(ws + L.idx[0]), (int*)(ws + L.idx[1]), (int*)(ws + L.idx[2])};
    int* gidx[2] = {(int*)(ws + L.gidx[0]), (int*)(ws + L.gidx[1])};
    unsigned char* taken = (unsigned char*)(ws + L.taken);
    unsigned* hist = (unsigned*)(ws + L.hist);
    unsigned* tot = (unsigned*)(ws + L.tot);
    int* ndet = (int*)(ws + L.ndet);
    hipStream_t st = (hipStream_t)stream;
    VocIn a;
    a.scores = scores; a.boxes = boxes; a.det_cls = det_cls; a.det_img = det_img; a.gt = gt_rows; a.gt_img = gt_img;
    a.D = D; a.G = G; a.I = I; a.C = C;

    if (int e = zero_async(tot, L.ndet + (size_t)(C + 1) * 4 - L.tot, st)) return e;          // tot .. ndet
    if (int e = zero_async(npos_out, (size_t)C * 4, st)) return e;
    const int nmax = D > G ? D : G;
    if (nmax > 0)
        hipLaunchKernelGGL(voc_init_kernel, dim3((nmax + VE_TILE - 1) / VE_TILE), dim3(VE_THREADS), 0, st, a, tp_out, idx[0], gidx[0], taken, ndet,
                           npos_out);
    // a stable LSD radix sort of an index list, 8 bits per pass: the first pass reads `src` and writes `a0`, the later ones alternate a0 -> a1 -> a0;
    // returns the buffer that holds the result.  Passes: score 4 + class <= 2 + image <= 3 + GT <= 4 = 13 <= VE_MAX_PASSES digit-total rows
    int pass = 0;
    auto radix = [&](int mode, int nbits, int n, int* src, int* a0, int* a1) -> int* {
        if (n == 0) return src;
        const int nb = (n + VE_TILE - 1) / VE_TILE;
        int* cur = src;
        for (int shift = 0; shift < nbits; shift += 8, ++pass) {
            int* dst = cur == a0 ? a1 : a0;
            unsigned* tp = tot + (size_t)256 * pass;
            hipLaunchKernelGGL(voc_radix_hist_kernel, dim3(nb), dim3(VE_THREADS), 0, st, a, mode, shift, cur, n, nb, hist, tp);
            hipLaunchKernelGGL(voc_radix_scan_kernel, dim3(256), dim3(VE_THREADS), 0, st, hist, nb, tp);
            hipLaunchKernelGGL(voc_radix_scatter_kernel, dim3(nb), dim3(VE_THREADS), 0, st, a, mode, shift, cur, dst, n, nb, hist);
            cur = dst;
        }
        return cur;
    };
    // sort A (per-class rank order): score bits first, then the class key [0, C]
    int* p1 = radix(KEY_SCORE, 32, D, idx[0], idx[1], idx[0]);
    p1 = radix(KEY_CLASS, bits_for(C), D, p1, p1 == idx[0] ? idx[1] : idx[0], p1);
    // sort B ((image, class) segments): the order of A by image, in the two buffers that do not hold A
    int* fb[2];
    for (int k = 0, m = 0; k < 3; ++k) if (idx[k] != p1) fb[m++] = idx[k];
    int* p2 = radix(KEY_IMAGE, bits_for(I - 1), D, p1, fb[0], fb[1]);
    // sort G: GT rows by the (image, class) key
    const int* g = radix(KEY_GT, bits_for((long long)I * (C + 1) - 1), G, gidx[0], gidx[1], gidx[0]);
    if (D > 0)
        hipLaunchKernelGGL(voc_match_kernel, dim3((D + VE_THREADS - 1) / VE_THREADS), dim3(VE_THREADS), 0, st, a, p2, g, taken, iou_thr, tp_out);
    hipLaunchKernelGGL(voc_ap_kernel, dim3(C), dim3(VE_THREADS), 0, st, a, p1, ndet, npos_out, tp_out, metric, ap_out);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}
