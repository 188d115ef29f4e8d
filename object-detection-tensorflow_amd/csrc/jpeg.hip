// JPEG decode for the data loader (include/odtk.h, "JPEG").  The serial half -- markers and Huffman decoding -- is host code in jpeg_host.h; this file
// binds it to the C-ABI and holds the regular per-block half as two kernels:
//   jpeg_idct_kernel    int16 coefficients x uint16 table -> f32, 8x8 inverse DCT (row pass and column pass meet in LDS), u8 sample planes on the padded
//                       block grids (scratch).  A workgroup takes 16 consecutive blocks = 2 KiB of coefficients: 8-byte loads, 4-byte stores.
//   jpeg_colour_kernel  triangle-filter chroma upsampling, YCbCr -> RGB, crop to width x height, u8 HWC.  A thread takes 4 consecutive pixels of the
//                       picture's raster = 12 bytes = three aligned dword stores.
// Both grids run over work units of the whole batch (16 blocks / 1024 pixels), found per picture from the running sums in the plans: a fixed number of
// workgroups strides over all units, so a large picture among small ones is shared by every workgroup.
#include "common.h"
#include "jpeg_host.h"

namespace {

constexpr int JPEG_THREADS = 256;
constexpr int JPEG_UNIT_BLOCKS = 16;
constexpr int JPEG_TILE_PX = 1024;

// 0.5 C(u) cos((2x + 1) u pi / 16) rounded to float32, [u][x]
static __device__ const float kBasis[64] = {
    0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f, 0.353553385f,
    0.490392625f, 0.415734798f, 0.277785122f, 0.0975451618f, -0.0975451618f, -0.277785122f, -0.415734798f, -0.490392625f,
    0.461939752f, 0.191341713f, -0.191341713f, -0.461939752f, -0.461939752f, -0.191341713f, 0.191341713f, 0.461939752f,
    0.415734798f, -0.0975451618f, -0.490392625f, -0.277785122f, 0.277785122f, 0.490392625f, 0.0975451618f, -0.415734798f,
    0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f, 0.353553385f, -0.353553385f, -0.353553385f, 0.353553385f,
    0.277785122f, -0.490392625f, 0.0975451618f, 0.415734798f, -0.415734798f, -0.0975451618f, 0.490392625f, -0.277785122f,
    0.191341713f, -0.461939752f, 0.461939752f, -0.191341713f, -0.191341713f, 0.461939752f, -0.461939752f, 0.191341713f,
    0.0975451618f, -0.277785122f, 0.415734798f, -0.490392625f, 0.490392625f, -0.415734798f, 0.277785122f, -0.0975451618f};

// the picture whose units hold unit u: the last plan with start <= u (starts are non-decreasing; a plan without units is never picked for a unit of a later one)
template <bool TILES>
__device__ inline int jpeg_find_plan(const odtk_jpeg_plan* __restrict__ plans, int N, int u) {
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int start = TILES ? plans[mid].tile_start : plans[mid].unit_start;
        if (start <= u) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline int jpeg_sample(float f) {
    const int s = (int)rintf(fminf(fmaxf(f, -1024.f), 1024.f)) + 128;      // (bounded first: hostile coefficients reach 1e11)
    return min(max(s, 0), 255);
}

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_idct_kernel(const odtk_jpeg_plan* __restrict__ plans, int N) {
    __shared__ float sF[JPEG_UNIT_BLOCKS * 64];
    __shared__ float sG[JPEG_UNIT_BLOCKS * 64];
    __shared__ float sB[64];
    const int t = threadIdx.x;
    if (t < 64) sB[t] = kBasis[t];
    const int total = plans[N - 1].unit_start + plans[N - 1].unit_count;
    const int bi = t >> 4, part = t & 15;          // block of the unit; 4 of its 64 values: row part / 2, columns 4 (part % 2) ..
    const int row = part >> 1, x0 = (part & 1) * 4;
    for (int u = blockIdx.x; u < total; u += gridDim.x) {
        const odtk_jpeg_plan& P = plans[jpeg_find_plan<false>(plans, N, u)];
        const int blk = (u - P.unit_start) * JPEG_UNIT_BLOCKS + bi;
        const bool live = u - P.unit_start < P.unit_count && blk < P.block_start[P.ncomp];
        int c = 0;
        if (live) {
            if (P.ncomp == 3) c = blk >= P.block_start[2] ? 2 : (blk >= P.block_start[1] ? 1 : 0);
            const uint2 cw = *reinterpret_cast<const uint2*>(P.coef + (size_t)blk * 64 + part * 4);
            const uint2 qw = *reinterpret_cast<const uint2*>(P.qtables + (P.tq[c] & 3) * 64 + part * 4);
            const int c0 = (int)(short)(cw.x & 0xffffu), c1 = (int)(short)(cw.x >> 16), c2 = (int)(short)(cw.y & 0xffffu), c3 = (int)(short)(cw.y >> 16);
            float* f = sF + bi * 64 + part * 4;
            f[0] = (float)(c0 * (int)(qw.x & 0xffffu));
            f[1] = (float)(c1 * (int)(qw.x >> 16));
            f[2] = (float)(c2 * (int)(qw.y & 0xffffu));
            f[3] = (float)(c3 * (int)(qw.y >> 16));
        }
        __syncthreads();
        if (live) {      // rows: g[v][x] = sum_u F[v][u] basis[u][x]
            const float* f = sF + bi * 64 + row * 8;
            float g[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < 8; ++k) {
                const float fk = f[k];
                for (int j = 0; j < 4; ++j) g[j] = g[j] + fk * sB[k * 8 + x0 + j];
            }
            for (int j = 0; j < 4; ++j) sG[bi * 64 + row * 8 + x0 + j] = g[j];
        }
        __syncthreads();
        if (live) {      // columns: f[y][x] = sum_v basis[v][y] g[v][x]
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            for (int k = 0; k < 8; ++k) {
                const float bk = sB[k * 8 + row];
                for (int j = 0; j < 4; ++j) o[j] = o[j] + bk * sG[bi * 64 + k * 8 + x0 + j];
            }
            const unsigned word = (unsigned)jpeg_sample(o[0]) | ((unsigned)jpeg_sample(o[1]) << 8) | ((unsigned)jpeg_sample(o[2]) << 16) |
                                  ((unsigned)jpeg_sample(o[3]) << 24);
            const int lb = blk - P.block_start[c], bw = P.blocks_w[c];
            const int by = lb / bw, bx = lb - by * bw;
            unsigned char* dst = P.planes + (size_t)P.block_start[c] * 64 + ((size_t)(by * 8 + row) * bw + bx) * 8 + x0;
            *reinterpret_cast<unsigned*>(dst) = word;
        }
        // (the next round writes sF behind this round's second barrier and sG behind its own first one: no third barrier)
    }
}

__device__ inline unsigned jpeg_u8(float v) { return (unsigned)min(max((int)rintf(v), 0), 255); }

__global__ void __launch_bounds__(JPEG_THREADS) jpeg_colour_kernel(const odtk_jpeg_plan* __restrict__ plans, int N) {
    const int t = threadIdx.x;
    const int total = plans[N - 1].tile_start + plans[N - 1].tile_count;
    for (int u = blockIdx.x; u < total; u += gridDim.x) {
        const odtk_jpeg_plan& P = plans[jpeg_find_plan<true>(plans, N, u)];
        const int w = P.width, h = P.height;
        const long long npx = (long long)w * h;
        const long long px0 = (long long)(u - P.tile_start) * JPEG_TILE_PX + t * 4;
        if (u - P.tile_start >= P.tile_count || px0 >= npx) continue;
        const int cnt = (int)(npx - px0 < 4 ? npx - px0 : 4);
        const int pitch_y = P.blocks_w[0] * 8;
        const bool colour = P.ncomp == 3;
        const int hs = P.hs, vs = P.vs;
        const int cwid = (w + hs - 1) / hs, chgt = (h + vs - 1) / vs;
        const int pitch_c = colour ? P.blocks_w[1] * 8 : 0;
        const unsigned char* pl_y = P.planes;
        const unsigned char* pl_cb = P.planes + (size_t)P.block_start[colour ? 1 : 0] * 64;
        const unsigned char* pl_cr = P.planes + (size_t)P.block_start[colour ? 2 : 0] * 64;
        int y = (int)(px0 / w), x = (int)(px0 - (long long)y * w);
        unsigned char rgb[12];
        for (int j = 0; j < 4; ++j) {
            unsigned r = 0, g = 0, b = 0;
            if (j < cnt) {
                const float Y = (float)pl_y[(size_t)y * pitch_y + x];
                if (!colour) {
                    r = g = b = (unsigned)Y;
                } else {
                    int cx = x, nx = x, cy = y, ny = y;
                    if (hs == 2) { cx = x >> 1; nx = (x & 1) ? min(cx + 1, cwid - 1) : max(cx - 1, 0); }
                    if (vs == 2) { cy = y >> 1; ny = (y & 1) ? min(cy + 1, chgt - 1) : max(cy - 1, 0); }
                    const size_t o_nn = (size_t)cy * pitch_c + cx, o_nf = (size_t)cy * pitch_c + nx, o_fn = (size_t)ny * pitch_c + cx, o_ff = (size_t)ny * pitch_c + nx;
                    const int cb16 = 3 * (3 * (int)pl_cb[o_nn] + (int)pl_cb[o_nf]) + (3 * (int)pl_cb[o_fn] + (int)pl_cb[o_ff]);
                    const int cr16 = 3 * (3 * (int)pl_cr[o_nn] + (int)pl_cr[o_nf]) + (3 * (int)pl_cr[o_fn] + (int)pl_cr[o_ff]);
                    const float cb = (float)cb16 * 0.0625f - 128.f, cr = (float)cr16 * 0.0625f - 128.f;      // exact sixteenths
                    r = jpeg_u8(Y + 1.402f * cr);
                    g = jpeg_u8((Y - 0.344136f * cb) - 0.714136f * cr);
                    b = jpeg_u8(Y + 1.772f * cb);
                }
                if (++x == w) { x = 0; ++y; }
            }
            rgb[3 * j] = (unsigned char)r; rgb[3 * j + 1] = (unsigned char)g; rgb[3 * j + 2] = (unsigned char)b;
        }
        unsigned char* dst = P.out + px0 * 3;       // px0 % 4 == 0: 12-byte steps from a 4-byte aligned base
        if (cnt == 4) {
            unsigned* d32 = reinterpret_cast<unsigned*>(dst);
            for (int k = 0; k < 3; ++k)
                d32[k] = (unsigned)rgb[4 * k] | ((unsigned)rgb[4 * k + 1] << 8) | ((unsigned)rgb[4 * k + 2] << 16) | ((unsigned)rgb[4 * k + 3] << 24);
        } else {
            for (int k = 0; k < 3 * cnt; ++k) dst[k] = rgb[k];
        }
    }
}

}  // namespace

extern "C" int odtk_jpeg_info(const void* data, size_t nbytes, struct odtk_jpeg_info* info) {
    char err[512];
    const int rc = odtk_jpeg::info((const unsigned char*)data, nbytes, info, err, sizeof(err));
    if (rc) odtk::set_error("%s", err);
    return rc;
}

extern "C" int odtk_jpeg_entropy_decode(const void* data, size_t nbytes, int16_t* coef, size_t coef_capacity, uint16_t* qtables) {
    char err[512];
    const int rc = odtk_jpeg::entropy_decode((const unsigned char*)data, nbytes, coef, coef_capacity, qtables, err, sizeof(err));
    if (rc) odtk::set_error("%s", err);
    return rc;
}

extern "C" int odtk_jpeg_plan_init(odtk_jpeg_plan* plan, const struct odtk_jpeg_info* info, const void* coef_dev, const void* qtables_dev, void* planes_dev,
                                   void* out_dev, int unit_start, int tile_start) {
    ODTK_REQUIRE(plan && info && coef_dev && qtables_dev && planes_dev && out_dev, "jpeg_plan_init: null pointer");
    ODTK_REQUIRE(((uintptr_t)coef_dev & 7) == 0 && ((uintptr_t)qtables_dev & 7) == 0 && ((uintptr_t)planes_dev & 15) == 0 && ((uintptr_t)out_dev & 3) == 0,
                 "jpeg_plan_init: coef / qtables need 8-byte, planes 16-byte, out 4-byte alignment");
    const int w = info->width, h = info->height, nc = info->ncomp;
    ODTK_REQUIRE(w >= 1 && w <= 65535 && h >= 1 && h <= 65535 && (nc == 1 || nc == 3), "jpeg_plan_init: %d x %d x %d out of range", w, h, nc);
    const int hs = nc == 1 ? 1 : info->hsamp[0], vs = nc == 1 ? 1 : info->vsamp[0];
    ODTK_REQUIRE((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2), "jpeg_plan_init: luma sampling %d x %d not supported", hs, vs);
    ODTK_REQUIRE(unit_start >= 0 && tile_start >= 0, "jpeg_plan_init: negative running sum");
    memset(plan, 0, sizeof(*plan));
    plan->coef = (const int16_t*)coef_dev; plan->qtables = (const uint16_t*)qtables_dev;
    plan->planes = (unsigned char*)planes_dev; plan->out = (unsigned char*)out_dev;
    plan->width = w; plan->height = h; plan->ncomp = nc; plan->hs = hs; plan->vs = vs;
    const int mcu_w = (w + 8 * hs - 1) / (8 * hs), mcu_h = (h + 8 * vs - 1) / (8 * vs);
    long long blocks = 0;
    for (int c = 0; c < nc; ++c) {
        ODTK_REQUIRE(info->tq[c] >= 0 && info->tq[c] <= 3, "jpeg_plan_init: quantisation table %d", info->tq[c]);
        plan->tq[c] = info->tq[c];
        plan->blocks_w[c] = mcu_w * (c == 0 ? hs : 1);
        plan->blocks_h[c] = mcu_h * (c == 0 ? vs : 1);
        plan->block_start[c] = (int)blocks;
        blocks += (long long)plan->blocks_w[c] * plan->blocks_h[c];
    }
    ODTK_REQUIRE(64 * blocks == info->coef_count, "jpeg_plan_init: info is not what odtk_jpeg_info wrote (coef_count %lld, geometry gives %lld)", info->coef_count,
                 64 * blocks);
    for (int c = nc; c < 4; ++c) plan->block_start[c] = (int)blocks;
    const long long units = (blocks + JPEG_UNIT_BLOCKS - 1) / JPEG_UNIT_BLOCKS, tiles = ((long long)w * h + JPEG_TILE_PX - 1) / JPEG_TILE_PX;
    ODTK_REQUIRE(unit_start + units < (1ll << 30) && tile_start + tiles < (1ll << 30), "jpeg_plan_init: batch too large");
    plan->unit_start = unit_start; plan->unit_count = (int)units;
    plan->tile_start = tile_start; plan->tile_count = (int)tiles;
    return ODTK_OK;
}

extern "C" int odtk_jpeg_reconstruct(const odtk_jpeg_plan* plans_dev, int N, void* stream) {
    ODTK_REQUIRE(plans_dev != nullptr, "jpeg_reconstruct: null plans");
    ODTK_REQUIRE(N >= 1 && N <= (1 << 20), "jpeg_reconstruct: N=%d out of range", N);
    hipStream_t st = (hipStream_t)stream;
    const int grid = N * 64 < 4096 ? N * 64 : 4096;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(grid), dim3(JPEG_THREADS), 0, st, plans_dev, N);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(grid), dim3(JPEG_THREADS), 0, st, plans_dev, N);
    ODTK_LAUNCH_CHECK();
    return ODTK_OK;
}
