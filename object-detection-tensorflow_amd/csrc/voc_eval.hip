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
//
// COCO-style AP (odtk_coco_eval; semantics in include/odtk.h, restated by tests/coco_eval_ref.py) shares init and the three sorts and replaces the tail:
//   gt prep  per sorted GT position: corners and h * w in f32 (the matcher reads them without the index indirection), npos[r][c] by integer atomics
//   match    one wave per 64 positions of sort B; the segment heads among them (a ballot) are taken one after the other, lane = (area range r,
//            IoU threshold t): box loads and the IoU are wave-uniform, the comparisons and the "matched" byte per (GT row, lane) are the lane's own
//            -> no cross-lane traffic inside a segment and no atomics; match_out[r][t][i] = 0 / 1 / 2
//   ap       one workgroup per (r, t, class): the backward chunk walk of voc_ap_kernel over the code-0 / code-1 positions; recall rises only at a
//            TP position, which contributes envelope x #{k : previous recall < x_k <= this recall} of the 101 recall points
//
// Ground-truth flags (odtk_voc_eval_flags / odtk_coco_eval_flags; gt_flags [G] bytes, NULL = all 0): 0 ordinary, 1 ignore (VOC `difficult`), 2 crowd.
// They are read in place, by GT row (init) or through the sorted GT index (gidx[m]: prep and the two matchers) -- no extra workspace.  init also checks
// the values: the largest row index + 1 with a flag above 2 goes by an integer atomicMax into a spare digit-total row of the workspace, which the
// entry point reads back (its only synchronisation, and only with gt_flags given) to refuse the call.  With gt_flags == NULL every kernel computes what
// it computed before the flags existed, bit for bit.
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
    const unsigned char* gfl;                             // per GT row: 0 ordinary, 1 ignore, 2 crowd; NULL = all 0
};
__device__ __forceinline__ int gt_flag(const VocIn& a, int j) { return a.gfl ? (int)a.gfl[j] : 0; }

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
                                                              int* ndet, int* npos, int* nign, int* bad) {
    __shared__ int hd[VE_MAX_CLASSES], hg[VE_MAX_CLASSES], hf[VE_MAX_CLASSES];      // valid detections, flag-0 GT rows, flagged GT rows
    const int t = threadIdx.x;
    for (int c = t; c < a.C; c += VE_THREADS) { hd[c] = 0; hg[c] = 0; hf[c] = 0; }
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
            const int f = gt_flag(a, i);
            if (f > 2) atomicMax(bad, i + 1);                              // not a flag: the entry point refuses the call
            if (c >= 0) atomicAdd(f ? &hf[c] : &hg[c], 1);
        }
    }
    __syncthreads();
    for (int c = t; c < a.C; c += VE_THREADS) {
        if (hd[c]) atomicAdd(&ndet[c], hd[c]);
        if (hg[c]) atomicAdd(&npos[c], hg[c]);
        if (nign && hf[c]) atomicAdd(&nign[c], hf[c]);
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
struct AddULL { __device__ unsigned long long operator()(unsigned long long x, unsigned long long y) const { return x + y; } };
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
        if (bj >= 0 && best > iou_thr) {
            if (gt_flag(a, gidx[bj])) {
                tp_out[i] = 2;                                              // on a flagged row: neither TP nor FP, and the row stays free
            } else if (!taken[bj]) {
                taken[bj] = 1;
                tp_out[i] = 1;
            }
        }
    }
}

// ---------------------------------------------------------------- AP per class
// a VOC match code as a pair of counts: TP in the low word, counted positions (TP or FP) in the high word; code 2 (on a flagged row) counts as neither
__device__ __forceinline__ unsigned long long voc_packed(int code) { return code == 1 ? ((1ull << 32) | 1ull) : (code == 0 ? (1ull << 32) : 0ull); }

// along the class's rank order the code-2 positions are skipped: precision = cumulative TP / counted positions so far (= the position + 1 without code 2)
__global__ void __launch_bounds__(VE_THREADS) voc_ap_kernel(VocIn a, const int* order, const int* ndet, const int* npos, const unsigned char* tp,
                                                            int metric, double* ap_out) {
    __shared__ int shi[VE_THREADS];
    __shared__ double shd[VE_THREADS];
    __shared__ unsigned long long shl[VE_THREADS];
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
    // total TP and counted positions of the class
    unsigned long long mine = 0;
    for (int k = t; k < n; k += VE_THREADS) mine += voc_packed(tp[order[start + k]]);
    mine = block_incl_scan(mine, shl, AddULL());
    if (t == VE_THREADS - 1) shl[0] = mine;
    __syncthreads();
    const unsigned long long total = shl[0];
    __syncthreads();
    const int total_tp = (int)(total & 0xffffffffull), total_cnt = (int)(total >> 32);
    const double dn = (double)np;
    double thr[11], pk[11];
    for (int k = 0; k < 11; ++k) { thr[k] = (double)k * 0.1; pk[k] = -1.0; }   // t_k = k * 0.1 in double: np.arange(0., 1.1, 0.1)
    unsigned long long after_carry = 0;                                     // TP / counted positions behind the current chunk
    double env_carry = 0.0;                                                 // max precision behind the current chunk (the sentinel 0 included)
    double area = 0.0;
    const int CH = VE_THREADS * VE_AP_ITEMS;
    for (int end = n; end > 0; end -= CH) {                                 // chunks from the back: [end - CH, end)
        const int s = end - CH;
        const int p0 = s + t * VE_AP_ITEMS;
        unsigned long long f[VE_AP_ITEMS];
        unsigned long long cnt = 0;
        for (int j = 0; j < VE_AP_ITEMS; ++j) {
            const int k = p0 + j;
            f[j] = (k >= 0 && k < end) ? voc_packed(tp[order[start + k]]) : 0ull;
            cnt += f[j];
        }
        // counts behind this thread's items: a suffix scan = a prefix scan over reversed threads
        const unsigned long long incl = block_incl_scan(cnt, shl, AddULL());  // (prefix over t; the suffix is chunk total - incl)
        if (t == VE_THREADS - 1) shl[0] = incl;
        __syncthreads();
        const unsigned long long chunk = shl[0];
        __syncthreads();
        unsigned long long after = after_carry + chunk - incl;             // (each word of incl <= the same word of chunk: no borrow)
        double prec[VE_AP_ITEMS];
        int tpc[VE_AP_ITEMS];
        double lmax = 0.0;
        for (int j = VE_AP_ITEMS - 1; j >= 0; --j) {
            tpc[j] = 0;
            prec[j] = 0.0;
            if (f[j]) {                                                     // a counted position (inside the chunk, code 0 or 1)
                after += f[j];
                tpc[j] = total_tp - (int)(after & 0xffffffffull) + (int)(f[j] & 1ull);   // cumulative TP up to and including this position
                const int upto = total_cnt - (int)(after >> 32) + 1;       // counted positions up to and including it
                prec[j] = (double)tpc[j] / fmax((double)upto, DBL_EPSILON);
                const double rec = (double)tpc[j] / dn;
                if (prec[j] > lmax) lmax = prec[j];
                for (int q = 0; q < 11; ++q)
                    if (rec >= thr[q] && prec[j] > pk[q]) pk[q] = prec[j];
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
            env = fmax(env, prec[j]);
            if (f[j] & 1ull) area += ((double)tpc[j] / dn - (double)(tpc[j] - 1) / dn) * env;
        }
        after_carry += chunk;
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

// ================================================================ COCO-style AP: every (area range, IoU threshold) pair in one pass
constexpr int CE_MAX_PAIRS = 64;                          // lanes of a wave: R * T <= 64

struct CocoPar {
    float thr[CE_MAX_PAIRS], lo[CE_MAX_PAIRS], hi[CE_MAX_PAIRS];          // thr[t], [lo[r], hi[r]]
    int T, R, max_dets;
};

// per sorted GT position m: corners (the expressions of voc_match_kernel) and the area h * w; npos[r][c] += 1 for every range that does not ignore the row
// (a flagged row is ignored in every range)
__global__ void __launch_bounds__(VE_THREADS) coco_gt_prep_kernel(VocIn a, CocoPar cp, const int* gidx, float4* gbox, float* garea, int* npos) {
    const int m = blockIdx.x * VE_THREADS + threadIdx.x;
    if (m >= a.G) return;
    const int j = gidx[m];
    const float* r = a.gt + (size_t)j * 5;
    const float yc = r[0], xc = r[1], h = r[2], w = r[3];
    gbox[m] = make_float4(yc - h / 2.f, xc - w / 2.f, yc + h / 2.f, xc + w / 2.f);
    const float ar = h * w;
    garea[m] = ar;
    const int c = gt_class(a, j);
    if (c < 0 || gt_flag(a, j)) return;
    for (int k = 0; k < cp.R; ++k)
        if (!(ar < cp.lo[k] || ar > cp.hi[k])) atomicAdd(&npos[k * a.C + c], 1);
}

// wave w owns positions [64 w, 64 w + 64) of the (image, class)-segmented order: the lanes find the heads among them (and the heads' GT ranges) in
// parallel, then the whole wave walks one head's segment at a time with lane = r * T + t.  matched: [G][R * T] bytes by sorted GT position, zeroed here
// for the segment's rows (a GT row belongs to one segment, a segment to one wave).  match_out was filled with 2.
// A row's flag is the same for every lane (m is wave-uniform): a flagged row is ignored in every range; a crowd row (2) takes intersection / detection
// area as its overlap -- one select on the denominator, the division and every other operation are those of the unflagged row -- and stays available
// however often it is matched.
__global__ void __launch_bounds__(VE_THREADS) coco_match_kernel(VocIn a, CocoPar cp, const int* order, const int* gidx, const float4* gbox,
                                                                const float* garea, unsigned char* matched, unsigned char* match_out) {
    const int lane = threadIdx.x & 63;
    const int base = (blockIdx.x * (VE_THREADS / 64) + (threadIdx.x >> 6)) * 64;
    const int p = base + lane;
    bool head = false;
    int g0 = 0, g1 = 0;
    if (p < a.D) {
        const int seg = det_segment(a, order[p]);
        head = (p == 0 || det_segment(a, order[p - 1]) != seg) && seg % (a.C + 1) != a.C;
        if (head) { g0 = gt_lower_bound(a, gidx, seg); g1 = gt_lower_bound(a, gidx, seg + 1); }
    }
    unsigned long long heads = __ballot(head);
    const int RT = cp.R * cp.T;
    const bool active = lane < RT;
    const int r = active ? lane / cp.T : 0, t = active ? lane % cp.T : 0;
    const float thr = cp.thr[t], lo = cp.lo[r], hi = cp.hi[r];
    while (heads) {                                                         // wave-uniform
        const int b = __ffsll((long long)heads) - 1;
        heads &= heads - 1ull;
        const int G0 = __shfl(g0, b), G1 = __shfl(g1, b);
        const int p0 = base + b;
        const int seg = det_segment(a, order[p0]);
        if (active)
            for (int m = G0; m < G1; ++m) matched[(size_t)m * RT + lane] = 0;
        for (int q = p0, k = 0; q < a.D && k < cp.max_dets; ++q, ++k) {
            const int i = order[q];
            if (q > p0 && det_segment(a, i) != seg) break;
            const float y1d = a.boxes[(size_t)i * 4 + 0], x1d = a.boxes[(size_t)i * 4 + 1];
            const float y2d = a.boxes[(size_t)i * 4 + 2], x2d = a.boxes[(size_t)i * 4 + 3];
            const float ad = (y2d - y1d) * (x2d - x1d);
            // the two candidates of the visiting order "non-ignored rows, then ignored rows": the best untaken non-ignored row wins if there is one
            float best_n = thr, best_i = thr;
            int m_n = -1, m_i = -1;
            for (int m = G0; m < G1; ++m) {
                const float4 gb = gbox[m];
                const float ag = garea[m];
                const float ih = fmaxf(fminf(y2d, gb.z) - fmaxf(y1d, gb.x), 0.f);
                const float iw = fmaxf(fminf(x2d, gb.w) - fmaxf(x1d, gb.y), 0.f);
                const float inter = ih * iw;
                const int fl = gt_flag(a, gidx[m]);
                const float uni = ad + (gb.z - gb.x) * (gb.w - gb.y) - inter;
                const float den = fl == 2 ? ad : uni;
                const float iou = den > 0.f ? inter / den : 0.f;
                if (!active || (fl != 2 && matched[(size_t)m * RT + lane])) continue;
                if (fl || ag < lo || ag > hi) {
                    if (!(iou < best_i)) { best_i = iou; m_i = m; }
                } else {
                    if (!(iou < best_n)) { best_n = iou; m_n = m; }
                }
            }
            if (!active) continue;
            const int mm = m_n >= 0 ? m_n : m_i;
            unsigned char code;
            if (mm >= 0) {
                matched[(size_t)mm * RT + lane] = 1;
                code = m_n >= 0 ? 1 : 2;
            } else {
                code = (ad < lo || ad > hi) ? 2 : 0;
            }
            match_out[(size_t)lane * a.D + i] = code;
        }
    }
}

// a match code as a pair of counts: TP in the low word, FP in the high word (n <= 8 Mi: no carry between them); code 2 counts as neither
__device__ __forceinline__ unsigned long long coco_packed(int code) { return code == 1 ? 1ull : (code == 0 ? (1ull << 32) : 0ull); }

// x_k = np.linspace(0, 1, 101)[k] as numpy builds it: k * (1 / 100) in double, the last one exactly 1
__device__ __forceinline__ double coco_recall_point(int k) { return k >= 100 ? 1.0 : (double)k * (1.0 / 100.0); }
// #{k in [0, 101) : x_k <= n / dn}: a guess from the quotient, then settled by the comparisons themselves
__device__ __forceinline__ int coco_points_upto(int n, double dn) {
    const double rec = (double)n / dn;
    int k = (int)(rec * 100.0) + 1;
    k = k < 0 ? 0 : (k > 101 ? 101 : k);
    while (k < 101 && rec >= coco_recall_point(k)) ++k;
    while (k > 0 && !(rec >= coco_recall_point(k - 1))) --k;
    return k;
}

// grid (C, R * T): AP and last recall of class c at pair (r, t) from the codes along the class's rank order (code 2 = not counted)
__global__ void __launch_bounds__(VE_THREADS) coco_ap_kernel(VocIn a, int T, const int* order, const int* ndet, const int* npos,
                                                             const unsigned char* match, double* ap_out, double* rec_out) {
    __shared__ int shi[VE_THREADS];
    __shared__ double shd[VE_THREADS];
    __shared__ unsigned long long shl[VE_THREADS];
    const int c = blockIdx.x, pair = blockIdx.y, t = threadIdx.x;
    const size_t out = (size_t)pair * a.C + c;
    int before = 0;
    for (int k = t; k < c; k += VE_THREADS) before += ndet[k];
    before = block_incl_scan(before, shi, AddI());
    if (t == VE_THREADS - 1) shi[0] = before;
    __syncthreads();
    const int start = shi[0], n = ndet[c], np = npos[(pair / T) * a.C + c];
    __syncthreads();
    if (np == 0) {
        if (t == 0) { ap_out[out] = __builtin_nan(""); rec_out[out] = __builtin_nan(""); }
        return;
    }
    const unsigned char* code = match + (size_t)pair * a.D;
    unsigned long long mine = 0;
    for (int k = t; k < n; k += VE_THREADS) mine += coco_packed(code[order[start + k]]);
    mine = block_incl_scan(mine, shl, AddULL());
    if (t == VE_THREADS - 1) shl[0] = mine;
    __syncthreads();
    const unsigned long long total = shl[0];
    __syncthreads();
    const int total_tp = (int)(total & 0xffffffffull), total_fp = (int)(total >> 32);
    const double dn = (double)np;
    unsigned long long after_carry = 0;                                     // counted positions behind the current chunk
    double env_carry = 0.0;                                                 // max precision behind the current chunk
    double sum = 0.0;
    const int CH = VE_THREADS * VE_AP_ITEMS;
    for (int end = n; end > 0; end -= CH) {                                 // chunks from the back: [end - CH, end)
        const int p0 = end - CH + t * VE_AP_ITEMS;
        unsigned long long f[VE_AP_ITEMS];
        unsigned long long cnt = 0;
        for (int j = 0; j < VE_AP_ITEMS; ++j) {
            const int k = p0 + j;
            f[j] = (k >= 0 && k < end) ? coco_packed(code[order[start + k]]) : 0ull;
            cnt += f[j];
        }
        const unsigned long long incl = block_incl_scan(cnt, shl, AddULL());
        if (t == VE_THREADS - 1) shl[0] = incl;
        __syncthreads();
        const unsigned long long chunk = shl[0];
        __syncthreads();
        unsigned long long after = after_carry + chunk - incl;             // (each word of incl <= the same word of chunk: no borrow)
        double prec[VE_AP_ITEMS];
        int tpc[VE_AP_ITEMS];
        double lmax = 0.0;
        for (int j = VE_AP_ITEMS - 1; j >= 0; --j) {
            tpc[j] = 0;
            prec[j] = 0.0;
            if (f[j]) {                                                     // a counted position: cumulative TP / FP up to and including it
                tpc[j] = total_tp - (int)(after & 0xffffffffull);
                const int fpc = total_fp - (int)(after >> 32);
                prec[j] = (double)tpc[j] / ((double)(tpc[j] + fpc) + DBL_EPSILON);
                if (prec[j] > lmax) lmax = prec[j];
                after += f[j];
            }
        }
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
            env = fmax(env, prec[j]);
            if (f[j] == 1ull) sum += env * (double)(coco_points_upto(tpc[j], dn) - coco_points_upto(tpc[j] - 1, dn));
        }
        after_carry += chunk;
        env_carry = fmax(env_carry, chunk_max);
    }
    shd[t] = sum;                                                           // fixed-order tree sum
    __syncthreads();
    for (int off = VE_THREADS / 2; off > 0; off >>= 1) {
        if (t < off) shd[t] = shd[t] + shd[t + off];
        __syncthreads();
    }
    if (t == 0) {
        // x_0 = 0 is reached at the first counted position, whose envelope is the maximum of all precisions (0 without counted positions)
        ap_out[out] = (shd[0] + env_carry) / 101.0;
        rec_out[out] = (double)total_tp / dn;
    }
}

int bits_for(long long maxval) {                                           // bits to represent 0..maxval
    int b = 0;
    while (b < 62 && (1ll << b) <= maxval) ++b;
    return b;
}
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct VocLayout {
    size_t idx[3], gidx[2], taken, hist, tot, bad, ndet, total;
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
    L.bad = L.tot + (size_t)256 * (VE_MAX_PASSES - 1) * 4;              // the last digit-total row: the sorts take 13 passes at the most (voc_sort)
    L.ndet = off; off += align256((size_t)(C + 1) * 4);
    L.total = off;
    return L;
}

bool voc_sizes_ok(int D, int G, int I, int C) {
    return D >= 0 && D <= VE_MAX_DET && G >= 0 && G <= VE_MAX_GT && I >= 1 && I <= VE_MAX_IMAGES && C >= 1 && C <= VE_MAX_CLASSES;
}
#define VOC_SIZES_MSG "voc_eval: num_det=%d num_gt=%d num_images=%d num_classes=%d outside the supported range (num_det <= %d, num_gt <= %d, " \
                      "1 <= num_images <= %d, 1 <= num_classes <= %d)"

// init and the three sorts on `st`: what odtk_voc_eval and odtk_coco_eval share.  flags_out [D] is zeroed, npos [C] receives the flag-0 GT rows per
// class, nign [C] (may be NULL) the flagged ones, the word at L.bad the check of the flag values (voc_flags_ok).
struct VocSorted {
    int* rank;        // sort A: the per-class global rank order
    int* seg;         // sort B: (image, class) segments, rank order inside each
    const int* gt;    // sort G: GT indices by the (image, class) key
    int* ndet;        // valid detections per class
};
int voc_sort(const VocIn& a, const VocLayout& L, char* ws, unsigned char* flags_out, int* npos, int* nign, hipStream_t st, VocSorted* out) {
    const int D = a.D, G = a.G, I = a.I, C = a.C;
    int* idx[3] = {(int*)(ws + L.idx[0]), (int*)(ws + L.idx[1]), (int*)(ws + L.idx[2])};
    int* gidx[2] = {(int*)(ws + L.gidx[0]), (int*)(ws + L.gidx[1])};
    unsigned char* taken = (unsigned char*)(ws + L.taken);
    unsigned* hist = (unsigned*)(ws + L.hist);
    unsigned* tot = (unsigned*)(ws + L.tot);
    int* ndet = (int*)(ws + L.ndet);
    if (int e = zero_async(tot, L.ndet + (size_t)(C + 1) * 4 - L.tot, st)) return e;          // tot .. ndet
    if (int e = zero_async(npos, (size_t)C * 4, st)) return e;
    if (nign)
        if (int e = zero_async(nign, (size_t)C * 4, st)) return e;
    const int nmax = D > G ? D : G;
    if (nmax > 0)
        hipLaunchKernelGGL(voc_init_kernel, dim3((nmax + VE_TILE - 1) / VE_TILE), dim3(VE_THREADS), 0, st, a, flags_out, idx[0], gidx[0], taken, ndet,
                           npos, nign, (int*)(ws + L.bad));
    // a stable LSD radix sort of an index list, 8 bits per pass: the first pass reads `src` and writes `a0`, the later ones alternate a0 -> a1 -> a0;
    // returns the buffer that holds the result.  Passes: score 4 + class <= 2 + image <= 3 + GT <= 4 = 13 < VE_MAX_PASSES digit-total rows (the last
    // row is never a pass's: its first word is L.bad)
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
    out->rank = p1;
    out->seg = radix(KEY_IMAGE, bits_for(I - 1), D, p1, fb[0], fb[1]);
    // sort G: GT rows by the (image, class) key
    out->gt = radix(KEY_GT, bits_for((long long)I * (C + 1) - 1), G, gidx[0], gidx[1], gidx[0]);
    out->ndet = ndet;
    return ODTK_OK;
}

// odtk_coco_eval's workspace: the VOC layout, then the GT rows by sorted position, the matched bytes and the scratch of the reused init kernel
struct CocoLayout {
    VocLayout v;
    size_t gbox, garea, matched, flags, npos_all, total;
};
CocoLayout coco_layout(int D, int G, int C, int RT) {
    CocoLayout L;
    L.v = voc_layout(D, G, C);
    size_t off = L.v.total;
    L.gbox = off; off += align256((size_t)G * 16);
    L.garea = off; off += align256((size_t)G * 4);
    L.matched = off; off += align256((size_t)G * RT);
    L.flags = off; off += align256((size_t)D);
    L.npos_all = off; off += align256((size_t)C * 4);
    L.total = off;
    return L;
}
bool coco_pairs_ok(int T, int R) { return T >= 1 && R >= 1 && (long long)T * R <= CE_MAX_PAIRS; }
// after the launches of a call with gt_flags: the word that init left at L.bad (0, or 1 + the largest row index whose flag is above 2) back on the
// host -- the one place where this file waits for the stream
int voc_flags_ok(const char* who, const char* ws, const VocLayout& L, hipStream_t st) {
    int bad = 0;
#ifdef __HIPCC__
    ODTK_CHECK_HIP(hipMemcpyAsync(&bad, ws + L.bad, sizeof(int), hipMemcpyDeviceToHost, st));
    ODTK_CHECK_HIP(hipStreamSynchronize(st));
#else                                                                       // the kernel source compiled for the host (tests): launches have run
    (void)st;
    memcpy(&bad, ws + L.bad, sizeof(int));
#endif
    ODTK_REQUIRE(bad == 0, "%s: gt_flags[%d] is above 2 (0 ordinary, 1 ignore, 2 crowd); the outputs are not valid", who, bad - 1);
    return ODTK_OK;
}
#define COCO_PAIRS_MSG "coco_eval: num_thr=%d num_areas=%d outside the supported range (1 <= num_thr, 1 <= num_areas, num_thr * num_areas <= %d)"

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
    return odtk_voc_eval_flags(scores, boxes, det_cls, det_img, num_det, gt_rows, gt_img, nullptr, num_gt, num_images, num_classes, iou_thr, metric,
                               workspace, tp_out, npos_out, nullptr, ap_out, stream);
}

extern "C" int odtk_voc_eval_flags(const float* scores, const float* boxes, const int* det_cls, const int* det_img, int num_det, const float* gt_rows,
                                   const int* gt_img, const unsigned char* gt_flags, int num_gt, int num_images, int num_classes, float iou_thr,
                                   int metric, void* workspace, unsigned char* match_out, int* npos_out, int* nign_out, double* ap_out, void* stream) {
    unsigned char* tp_out = match_out;
    ODTK_REQUIRE(voc_sizes_ok(num_det, num_gt, num_images, num_classes), VOC_SIZES_MSG, num_det, num_gt, num_images, num_classes, VE_MAX_DET,
                 VE_MAX_GT, VE_MAX_IMAGES, VE_MAX_CLASSES);
    ODTK_REQUIRE(metric == 0 || metric == 1, "voc_eval: metric %d (0 = voc07 11-point, 1 = area)", metric);
    ODTK_REQUIRE(workspace && npos_out && ap_out, "voc_eval: null pointer");
    ODTK_REQUIRE(num_det == 0 || (scores && boxes && det_cls && det_img && tp_out), "voc_eval: null detection pointer");
    ODTK_REQUIRE(num_gt == 0 || (gt_rows && gt_img), "voc_eval: null ground-truth pointer");
    const int D = num_det, G = num_gt, I = num_images, C = num_classes;
    const VocLayout L = voc_layout(D, G, C);
    hipStream_t st = (hipStream_t)stream;
    VocIn a;
    a.scores = scores; a.boxes = boxes; a.det_cls = det_cls; a.det_img = det_img; a.gt = gt_rows; a.gt_img = gt_img;
    a.D = D; a.G = G; a.I = I; a.C = C; a.gfl = G > 0 ? gt_flags : nullptr;
    VocSorted s;
    if (int e = voc_sort(a, L, (char*)workspace, tp_out, npos_out, nign_out, st, &s)) return e;
    if (D > 0)
        hipLaunchKernelGGL(voc_match_kernel, dim3((D + VE_THREADS - 1) / VE_THREADS), dim3(VE_THREADS), 0, st, a, s.seg, s.gt,
                           (unsigned char*)workspace + L.taken, iou_thr, tp_out);
    hipLaunchKernelGGL(voc_ap_kernel, dim3(C), dim3(VE_THREADS), 0, st, a, s.rank, s.ndet, npos_out, tp_out, metric, ap_out);
    ODTK_LAUNCH_CHECK();
    return a.gfl ? voc_flags_ok("voc_eval", (const char*)workspace, L, st) : ODTK_OK;
}

extern "C" long long odtk_coco_eval_workspace_bytes(int num_det, int num_gt, int num_images, int num_classes, int num_thr, int num_areas) {
    if (!voc_sizes_ok(num_det, num_gt, num_images, num_classes)) {
        set_error(VOC_SIZES_MSG, num_det, num_gt, num_images, num_classes, VE_MAX_DET, VE_MAX_GT, VE_MAX_IMAGES, VE_MAX_CLASSES);
        return -1;
    }
    if (!coco_pairs_ok(num_thr, num_areas)) {
        set_error(COCO_PAIRS_MSG, num_thr, num_areas, CE_MAX_PAIRS);
        return -1;
    }
    return (long long)coco_layout(num_det, num_gt, num_classes, num_thr * num_areas).total;
}

extern "C" int odtk_coco_eval(const float* scores, const float* boxes, const int* det_cls, const int* det_img, int num_det, const float* gt_rows,
                              const int* gt_img, int num_gt, int num_images, int num_classes, const float* iou_thr, int num_thr,
                              const float* area_rng, int num_areas, int max_dets, void* workspace, unsigned char* match_out, int* npos_out,
                              double* ap_out, double* recall_out, void* stream) {
    return odtk_coco_eval_flags(scores, boxes, det_cls, det_img, num_det, gt_rows, gt_img, nullptr, num_gt, num_images, num_classes, iou_thr, num_thr,
                                area_rng, num_areas, max_dets, workspace, match_out, npos_out, ap_out, recall_out, stream);
}

extern "C" int odtk_coco_eval_flags(const float* scores, const float* boxes, const int* det_cls, const int* det_img, int num_det, const float* gt_rows,
                                    const int* gt_img, const unsigned char* gt_flags, int num_gt, int num_images, int num_classes,
                                    const float* iou_thr, int num_thr, const float* area_rng, int num_areas, int max_dets, void* workspace,
                                    unsigned char* match_out, int* npos_out, double* ap_out, double* recall_out, void* stream) {
    ODTK_REQUIRE(voc_sizes_ok(num_det, num_gt, num_images, num_classes), VOC_SIZES_MSG, num_det, num_gt, num_images, num_classes, VE_MAX_DET,
                 VE_MAX_GT, VE_MAX_IMAGES, VE_MAX_CLASSES);
    ODTK_REQUIRE(coco_pairs_ok(num_thr, num_areas), COCO_PAIRS_MSG, num_thr, num_areas, CE_MAX_PAIRS);
    ODTK_REQUIRE(max_dets >= 1, "coco_eval: max_dets %d (must be >= 1)", max_dets);
    ODTK_REQUIRE(iou_thr && area_rng && workspace && npos_out && ap_out && recall_out, "coco_eval: null pointer");
    ODTK_REQUIRE(num_det == 0 || (scores && boxes && det_cls && det_img && match_out), "coco_eval: null detection pointer");
    ODTK_REQUIRE(num_gt == 0 || (gt_rows && gt_img), "coco_eval: null ground-truth pointer");
    const int D = num_det, G = num_gt, C = num_classes, T = num_thr, R = num_areas, RT = T * R;
    const CocoLayout L = coco_layout(D, G, C, RT);
    char* ws = (char*)workspace;
    hipStream_t st = (hipStream_t)stream;
    VocIn a;
    a.scores = scores; a.boxes = boxes; a.det_cls = det_cls; a.det_img = det_img; a.gt = gt_rows; a.gt_img = gt_img;
    a.D = D; a.G = G; a.I = num_images; a.C = C; a.gfl = G > 0 ? gt_flags : nullptr;
    CocoPar cp;
    for (int k = 0; k < CE_MAX_PAIRS; ++k) {
        cp.thr[k] = k < T ? iou_thr[k] : 0.f;
        cp.lo[k] = k < R ? area_rng[2 * k] : 0.f;
        cp.hi[k] = k < R ? area_rng[2 * k + 1] : 0.f;
    }
    cp.T = T; cp.R = R; cp.max_dets = max_dets;
    VocSorted s;
    if (int e = voc_sort(a, L.v, ws, (unsigned char*)(ws + L.flags), (int*)(ws + L.npos_all), nullptr, st, &s)) return e;
    if (int e = zero_async(npos_out, (size_t)R * C * 4, st)) return e;
    float4* gbox = (float4*)(ws + L.gbox);
    float* garea = (float*)(ws + L.garea);
    if (G > 0)
        hipLaunchKernelGGL(coco_gt_prep_kernel, dim3((G + VE_THREADS - 1) / VE_THREADS), dim3(VE_THREADS), 0, st, a, cp, s.gt, gbox, garea, npos_out);
    if (D > 0) {
        ODTK_CHECK_HIP(hipMemsetAsync(match_out, 2, (size_t)RT * D, st));   // beyond max_dets, invalid: never visited by the matcher
        hipLaunchKernelGGL(coco_match_kernel, dim3((D + VE_THREADS - 1) / VE_THREADS), dim3(VE_THREADS), 0, st, a, cp, s.seg, s.gt, gbox, garea,
                           (unsigned char*)(ws + L.matched), match_out);
    }
    hipLaunchKernelGGL(coco_ap_kernel, dim3(C, RT), dim3(VE_THREADS), 0, st, a, T, s.rank, s.ndet, npos_out, match_out, ap_out, recall_out);
    ODTK_LAUNCH_CHECK();
    return a.gfl ? voc_flags_ok("coco_eval", ws, L.v, st) : ODTK_OK;
}
