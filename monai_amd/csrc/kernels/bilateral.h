// Exact bilateral filter: monai._C.bilateral_filter(input, spatial_sigma, color_sigma, fast_approx=False) (monai/csrc/ext.cpp:23, filtering/bilateral/bilateral.cpp,
// bilateralfilter_cpu.cpp:20-124; the reference's device form is CUDA only: bilateralfilter_cuda.cu).  B images of C channels [C][D][H][W]; per output voxel
//     out_c = sum_t w_t x_c[nb_t] / sum_t w_t,   w_t = prod_axes exp(-d_axis^2 / (2 sigma_s^2)) * exp(-sum_c (x_c[home] - x_c[nb_t])^2 / (2 sigma_c^2))
// over a window of K taps per axis, K = (int)ceil(5.0f * sigma_s) | 1 (the product in float32), neighbour indices clamped to the volume (replicate).  The colour
// distance is joint over the C channels: one weight per tap for all channels of a voxel.  An axis of extent 1 clamps every tap to the same voxel, so its K taps
// multiply numerator and denominator by the same factor: such an axis is given one tap (this is also how 1-D and 2-D images, passed with leading 1s, get their
// window).  The home tap has weight 1, so sum w >= 1.  A window that holds NaN, or +-inf in channel c, gives NaN (in every channel / in channel c) exactly as the
// reference's arithmetic does: exp(-inf) * inf.
//
//   bilateral_tile_kernel<C, LDSF>   float32, C = 1 .. 4.  A 256-lane workgroup stages its tile with the halo, all channels, in LDS; indices are clamped while
//                                    staging, the tap loops carry no bounds logic.  Staged values are pre-scaled by s = sqrt(log2(e) / (2 sigma_c^2)) and the spatial
//                                    weight is folded into the exponent: w = exp2(-(sum_c d_c^2 + g)), g = the sum of the per-axis d^2 log2(e) / (2 sigma_s^2) read
//                                    from a K-entry LDS table; per tap and channel-1 output: v_sub, v_fma, v_exp, v_fma, v_add.  A lane owns BIL_R = 4 consecutive
//                                    outputs along x and slides a register window along the row: one ds_read_b128 per channel and one (broadcast) of the table serve
//                                    4 taps x 4 outputs; the K % 4 last taps of a row read single values.  Sums live in registers, each output is written once and the
//                                    scale is taken out once at the end.  The lanes form a box 2^a (x) x 2^b (y) x 2^(8-a-b) (z) chosen by the host (bilateral_plan) to
//                                    minimise the staged tile; LDSF is the static tile size, 16 KiB or 63 KiB beside the 1 KiB table (the smaller lets more
//                                    workgroups share a CU).  Rows have a pitch that is a multiple of 4 floats, so every b128 read is 16-byte aligned.
//   bilateral_generic_kernel<T>      float and double, any K <= 255, any C <= 16: one output per thread, taps from global memory with clamped indices, the
//                                    reference's formulation (natural exponent of the summed arguments), sums in registers.
//
// No atomics, no read-modify-write of global memory; each output is written once by one thread: the same bits on every run.  Offsets across images and channels are
// 64-bit.  The tile path needs |x| s to stay finite in float32 (the host sends a colour sigma whose s or 1 / s is not a normal float to the generic kernel).
#pragma once
#include "common.h"

namespace mh {

enum { BIL_MAX_K = 255, BIL_MAX_C = 16, BIL_TILE_MAX_C = 4, BIL_R = 4, BIL_TAB = 260, BIL_LDS_SMALL = 4096, BIL_LDS_LARGE = 16384 - BIL_TAB };

__device__ __forceinline__ int bil_clamp(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }
// 2^v for v <= 0, one v_exp_f32: a result below 2^-126 is flushed to 0 (such a weight adds nothing to a sum that is at least 1), where exp2f() spends four more
// instructions per tap on scaling it into the denormal range.  The SIMT emulator of tests/emu has no such builtin and takes libm's exp2f.
#ifdef MH_SIMT_EMULATOR
__device__ __forceinline__ float bil_exp2(float v) { return exp2f(v); }
#else
__device__ __forceinline__ float bil_exp2(float v) { return __builtin_amdgcn_exp2f(v); }
#endif

struct BilTile {
    int D, H, W;
    int K, hz, hy, hx;        // taps per axis of extent > 1, half widths per axis (0 on an axis of extent 1)
    int la, lb;               // lanes: 2^la (x) * 2^lb (y) * 2^(8 - la - lb) (z); a lane owns BIL_R outputs along x
    int pitch, py, pz;        // staged rows of `pitch` floats (a multiple of 4, above the staged columns: the window reads one float past them), py rows, pz planes per channel
    int tiles_x, tiles_y;
    int vec;                  // every row of dst starts 16-byte aligned
    float ks, s, inv_s;       // log2(e) / (2 sigma_s^2); sqrt(log2(e) / (2 sigma_c^2)) and its inverse
};

// one tap of the row for the lane's 4 outputs: output j meets the value w[c][k + j]
template <int C>
__device__ __forceinline__ void bil_tap(const float (&hv)[C][BIL_R], const float (&w)[C][2 * BIL_R], const int k, const float g, float (&a)[C][BIL_R], float (&ws)[BIL_R]) {
#pragma unroll
    for (int j = 0; j < BIL_R; ++j) {
        float e = g;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float d = hv[c][j] - w[c][k + j];
            e = fmaf(d, d, e);
        }
        const float wt = bil_exp2(-e);
#pragma unroll
        for (int c = 0; c < C; ++c) a[c][j] = fmaf(wt, w[c][k + j], a[c][j]);
        ws[j] += wt;
    }
}

// grid (tiles_x * tiles_y * tiles_z, B), 256 threads; the staged tile C * pz * py * pitch <= LDSF floats (checked by the host)
template <int C, int LDSF>
__global__ void __launch_bounds__(256) bilateral_tile_kernel(const float* __restrict__ src, float* __restrict__ dst, BilTile g) {
    __shared__ __attribute__((aligned(16))) float tile[LDSF];
    __shared__ __attribute__((aligned(16))) float tab[BIL_TAB];
    const int tid = threadIdx.x;
    const int h = g.K >> 1;
    for (int i = tid; i < BIL_TAB; i += 256) {
        const float d = (float)(i - h);
        tab[i] = i < g.K ? d * d * g.ks : 0.0f;
    }
    const int tx = BIL_R << g.la, ty = 1 << g.lb, tz = 256 >> (g.la + g.lb);
    const int px = tx + 2 * g.hx, py = g.py, pz = g.pz, pitch = g.pitch;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % (unsigned)g.tiles_x) * tx;
    b /= (unsigned)g.tiles_x;
    const int y0 = (int)(b % (unsigned)g.tiles_y) * ty, z0 = (int)(b / (unsigned)g.tiles_y) * tz;
    const long long plane = (long long)g.H * g.W, chs = (long long)g.D * plane, image = (long long)blockIdx.y * C * chs;
    const float* img = src + image;
    {   // staging: 8 groups of 32 lanes, a group takes every 8th row (y, then z, then channel) and walks along x
        const int sl = tid & 31;
        int r = tid >> 5, p = 0, c = 0;
        while (r >= py) { r -= py; ++p; }
        while (p >= pz) { p -= pz; ++c; }
        while (c < C) {
            const int gy = bil_clamp(y0 - g.hy + r, g.H), gz = bil_clamp(z0 - g.hz + p, g.D);
            const float* in = img + c * chs + gz * plane + (long long)gy * g.W;
            float* out = tile + ((c * pz + p) * py + r) * pitch;
            for (int col = sl; col < px; col += 32) out[col] = in[bil_clamp(x0 - g.hx + col, g.W)] * g.s;
            r += 8;
            while (r >= py) { r -= py; ++p; }
            while (p >= pz) { p -= pz; ++c; }
        }
    }
    __syncthreads();
    const int lx = tid & ((1 << g.la) - 1), ly = (tid >> g.la) & (ty - 1), lz = tid >> (g.la + g.lb);
    const int x = x0 + BIL_R * lx, y = y0 + ly, z = z0 + lz;
    if (x >= g.W || y >= g.H || z >= g.D) return;
    const int chf = pz * py * pitch;
    const float* base = tile + (lz * py + ly) * pitch + BIL_R * lx;      // the tap (0, 0, 0) of the lane's first output
    const float* home = base + (g.hz * py + g.hy) * pitch + g.hx;
    float hv[C][BIL_R], a[C][BIL_R], ws[BIL_R];
#pragma unroll
    for (int j = 0; j < BIL_R; ++j) {
        ws[j] = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) { hv[c][j] = home[c * chf + j]; a[c][j] = 0.0f; }
    }
    const int kz = 2 * g.hz + 1, ky = 2 * g.hy + 1, kx = 2 * g.hx + 1;
    const float* tabz = tab + (g.hz ? 0 : h);      // an axis with one tap reads the table's centre (0)
    const float* taby = tab + (g.hy ? 0 : h);
    const float* tabx = tab + (g.hx ? 0 : h);      // kx >= 4 implies hx == h: the b128 reads below start at tab
    for (int dz = 0; dz < kz; ++dz)
        for (int dy = 0; dy < ky; ++dy) {
            const float gzy = tabz[dz] + taby[dy];
            const float* row = base + (dz * py + dy) * pitch;
            float w[C][2 * BIL_R];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 t = *reinterpret_cast<const float4*>(row + c * chf);
                w[c][0] = t.x; w[c][1] = t.y; w[c][2] = t.z; w[c][3] = t.w;
            }
            int dx = 0;
            for (; dx + 4 <= kx; dx += 4) {
                const float4 gx = *reinterpret_cast<const float4*>(tab + dx);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float4 t = *reinterpret_cast<const float4*>(row + c * chf + dx + 4);
                    w[c][4] = t.x; w[c][5] = t.y; w[c][6] = t.z; w[c][7] = t.w;
                }
                bil_tap<C>(hv, w, 0, gzy + gx.x, a, ws);
                bil_tap<C>(hv, w, 1, gzy + gx.y, a, ws);
                bil_tap<C>(hv, w, 2, gzy + gx.z, a, ws);
                bil_tap<C>(hv, w, 3, gzy + gx.w, a, ws);
#pragma unroll
                for (int c = 0; c < C; ++c) { w[c][0] = w[c][4]; w[c][1] = w[c][5]; w[c][2] = w[c][6]; w[c][3] = w[c][7]; }
            }
            for (; dx < kx; ++dx) {
                bil_tap<C>(hv, w, 0, gzy + tabx[dx], a, ws);
#pragma unroll
                for (int c = 0; c < C; ++c) { w[c][0] = w[c][1]; w[c][1] = w[c][2]; w[c][2] = w[c][3]; w[c][3] = row[c * chf + dx + 4]; }
            }
        }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float* out = dst + image + c * chs + z * plane + (long long)y * g.W + x;
        float o[BIL_R];
#pragma unroll
        for (int j = 0; j < BIL_R; ++j) o[j] = (a[c][j] / ws[j]) * g.inv_s;
        if (g.vec && x + BIL_R <= g.W) {
            *reinterpret_cast<float4*>(out) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < BIL_R; ++j)
                if (x + j < g.W) out[j] = o[j];
        }
    }
}

template <typename T>
struct BilGeneric {
    int C, D, H, W;
    int hz, hy, hx;
    T ks, kc;                 // 1 / (2 sigma_s^2), 1 / (2 sigma_c^2), each rounded to float32 first as the reference's constants are
};

__device__ __forceinline__ float bil_exp(float v) { return expf(v); }
__device__ __forceinline__ double bil_exp(double v) { return exp(v); }

// grid (ceil(D H W / 256), B), 256 threads, one output voxel (all channels) per thread
template <typename T>
__global__ void __launch_bounds__(256) bilateral_generic_kernel(const T* __restrict__ src, T* __restrict__ dst, BilGeneric<T> g) {
    const long long plane = (long long)g.H * g.W, chs = (long long)g.D * plane, image = (long long)blockIdx.y * g.C * chs;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= chs) return;
    const int x = (int)(idx % g.W), y = (int)((idx / g.W) % g.H), z = (int)(idx / plane);
    const T* img = src + image;
    T hv[BIL_MAX_C], a[BIL_MAX_C], ws = (T)0;
#pragma unroll
    for (int c = 0; c < BIL_MAX_C; ++c) {
        a[c] = (T)0;
        hv[c] = c < g.C ? img[c * chs + idx] : (T)0;
    }
    for (int dz = -g.hz; dz <= g.hz; ++dz) {
        const long long oz = bil_clamp(z + dz, g.D) * plane;
        for (int dy = -g.hy; dy <= g.hy; ++dy) {
            const long long ozy = oz + (long long)bil_clamp(y + dy, g.H) * g.W;
            const T gzy = (T)(dz * dz + dy * dy);
            for (int dx = -g.hx; dx <= g.hx; ++dx) {
                const T* nb = img + ozy + bil_clamp(x + dx, g.W);
                T v[BIL_MAX_C], e = (T)0;
#pragma unroll
                for (int c = 0; c < BIL_MAX_C; ++c)
                    if (c < g.C) {
                        v[c] = nb[c * chs];
                        const T d = hv[c] - v[c];
                        e += d * d;
                    }
                const T wt = bil_exp(-(e * g.kc + (gzy + (T)(dx * dx)) * g.ks));
#pragma unroll
                for (int c = 0; c < BIL_MAX_C; ++c)
                    if (c < g.C) a[c] += v[c] * wt;
                ws += wt;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < BIL_MAX_C; ++c)
        if (c < g.C) dst[image + c * chs + idx] = a[c] / ws;
}

}  // namespace mh
