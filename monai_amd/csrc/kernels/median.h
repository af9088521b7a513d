// Exact median filter over a box window with replicate padding: MedianSmooth(d) / MedianFilter / median_filter (monai/networks/layers/simplelayers.py:441-539: replicate
// F.pad, a one-hot conv3d that writes every voxel's whole window as k^3 channels, torch.median over them).  n independent fp32 images [D][H][W], radii (rz, ry, rx),
// window (2 rz + 1)(2 ry + 1)(2 rx + 1) <= MED_MAX_WINDOW values, always odd: the median is the middle order statistic, a selection -- no rounding anywhere.
//
// What the reference's arithmetic does to special values is reproduced (the one-hot convolution multiplies every window value by 0 or 1 and adds them up from +0):
//   * a selected -0.0 comes out as +0.0: zeros are stored as +0.0 when the tile is staged;
//   * a window that holds +-inf or NaN gives NaN (inf * 0): non-finite values are marked when the tile is staged and counted per window.
//
//   median3_kernel<RZ>     radius 1 in x and y, RZ (0 or 1) in z: 9 or 27 values, selected in registers with min / max / v_med3_f32 only.  A workgroup stages its
//                          input tile with the halo in LDS (row pitch odd); a lane owns one row (y) and marches MED_TX outputs along x: per step it reads the new
//                          3 (y) x (2 RZ + 1) (z) column from LDS, sorts it (25 exchanges for 9 values), and selects from the three sorted columns it holds -- two of
//                          them are the previous outputs' columns.  Lanes run along y so that the LDS reads of a wave walk consecutive rows of odd pitch: no bank
//                          conflict.  From three sorted 9-columns A, B, C: sort every rank across the columns (lo_i <= md_i <= hi_i); in that 9 x 3 arrangement with
//                          sorted rows and columns the entry of rank i and place j has (i + 1)(j + 1) - 1 entries below and (9 - i)(3 - j) - 1 above it, which rules
//                          out all but lo_5..8, md_2..6, hi_0..3 -- 7 entries go on each side, so the median of the 27 is the median of those 13, found by
//                          dropping the minimum and the maximum of 8, 7, ... 4 of them in turn.  MED_TX = 16 is measured (512^3: 0.90 ms against 1.33 ms at 32 and
//                          0.96 ms at 8): the smaller tile lets 5 workgroups share a CU instead of 2.
//   median_general_kernel  any radii: a workgroup stages order-preserving 32-bit keys of its tile with the halo in LDS; one thread per output finds the largest t with
//                          #{window keys < t} <= window / 2 -- the key of the median -- two bits per pass, 16 passes over the window in LDS, the same trip counts in
//                          every lane.  The 256 outputs of a workgroup form a box 2^a x 2^b x 2^c chosen by the host to minimise the staged tile.
//
// No atomics; each output is written once by one thread: the same bits on every run.  Offsets into an image and across images are 64-bit.
#pragma once
#include "common.h"

namespace mh {

enum { MED_MAX_WINDOW = 343, MED_TX = 16, MED_PITCH = MED_TX + 3, MED_FAST_LDS = 6 * 66 * MED_PITCH, MED_GEN_LDS = 2048 };
constexpr unsigned MED_BAD_KEY = 0xffffffffu;      // above the key of every finite value (0xff7fffff at most)

__device__ __forceinline__ bool med_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ int med_clamp(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }
__device__ __forceinline__ void med_cx(float& a, float& b) {      // compare-exchange: a <= b afterwards
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}
__device__ __forceinline__ float med_min3(float a, float b, float c) { return fminf(fminf(a, b), c); }
__device__ __forceinline__ float med_max3(float a, float b, float c) { return fmaxf(fmaxf(a, b), c); }

// the optimal 25-exchange network for 9 values (7 layers)
__device__ __forceinline__ void med_sort9(float* v) {
    med_cx(v[0], v[3]); med_cx(v[1], v[7]); med_cx(v[2], v[5]); med_cx(v[4], v[8]);
    med_cx(v[0], v[7]); med_cx(v[2], v[4]); med_cx(v[3], v[8]); med_cx(v[5], v[6]);
    med_cx(v[0], v[2]); med_cx(v[1], v[3]); med_cx(v[4], v[5]); med_cx(v[7], v[8]);
    med_cx(v[1], v[4]); med_cx(v[3], v[6]); med_cx(v[5], v[7]);
    med_cx(v[0], v[1]); med_cx(v[2], v[4]); med_cx(v[3], v[5]); med_cx(v[6], v[8]);
    med_cx(v[2], v[3]); med_cx(v[4], v[5]); med_cx(v[6], v[7]);
    med_cx(v[1], v[2]); med_cx(v[3], v[4]); med_cx(v[5], v[6]);
}

// minimum of v[0 .. N) to v[0], maximum to v[N - 1]; the values in between stay a permutation of the rest
template <int N>
__device__ __forceinline__ void med_ends(float* v) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) med_cx(v[i], v[N - 1 - i]);
#pragma unroll
    for (int i = 1; i < (N + 1) / 2; ++i) med_cx(v[0], v[i]);
#pragma unroll
    for (int i = N / 2; i < N - 1; ++i) med_cx(v[i], v[N - 1]);
}

// median of 13 values (destroys them): the minimum and the maximum of any 8 are not the median, ...
__device__ __forceinline__ float med_median13(float* v) {
    med_ends<8>(v);             // v[1 .. 7) + v[8]
    v[7] = v[8];
    med_ends<7>(v + 1);         // v[2 .. 7) + v[9]
    v[7] = v[9];
    med_ends<6>(v + 2);         // v[3 .. 7) + v[10]
    v[7] = v[10];
    med_ends<5>(v + 3);         // v[4 .. 7) + v[11]
    v[7] = v[11];
    med_ends<4>(v + 4);         // v[5 .. 7) + v[12]
    return __builtin_amdgcn_fmed3f(v[5], v[6], v[12]);
}

// median of the 27 values of three sorted 9-columns
__device__ __forceinline__ float med_select27(const float* a, const float* b, const float* c) {
    float v[13];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = med_min3(a[5 + i], b[5 + i], c[5 + i]);
#pragma unroll
    for (int i = 0; i < 5; ++i) v[4 + i] = __builtin_amdgcn_fmed3f(a[2 + i], b[2 + i], c[2 + i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[9 + i] = med_max3(a[i], b[i], c[i]);
    return med_median13(v);
}
// median of the 9 values of three sorted 3-columns
__device__ __forceinline__ float med_select9(const float* a, const float* b, const float* c) {
    return __builtin_amdgcn_fmed3f(med_max3(a[0], b[0], c[0]), __builtin_amdgcn_fmed3f(a[1], b[1], c[1]), med_min3(a[2], b[2], c[2]));
}

// one column of the staged tile: NZ planes x 3 rows at `p`, sorted; returns whether it holds a marked (non-finite) value
template <int NZ, int PLANE>
__device__ __forceinline__ bool med_column(const float* p, float* v) {
    bool bad = false;
#pragma unroll
    for (int z = 0; z < NZ; ++z)
#pragma unroll
        for (int y = 0; y < 3; ++y) {
            const float t = p[z * PLANE + y * MED_PITCH];
            bad |= t != t;
            v[z * 3 + y] = t;
        }
    if (NZ == 3) {
        med_sort9(v);
    } else {
        const float lo = med_min3(v[0], v[1], v[2]), md = __builtin_amdgcn_fmed3f(v[0], v[1], v[2]), hi = med_max3(v[0], v[1], v[2]);
        v[0] = lo; v[1] = md; v[2] = hi;
    }
    return bad;
}

// grid (tiles_x * tiles_y * tiles_z, n), 256 threads.  RZ = 1: the 4 waves take 4 consecutive planes of 64 rows; RZ = 0: one plane, 256 rows.  vec: every row
// of dst starts 16-byte aligned (W % 4 == 0 and dst aligned)
template <int RZ>
__global__ void __launch_bounds__(256) median3_kernel(const float* __restrict__ src, float* __restrict__ dst, int D, int H, int W, int tiles_x, int tiles_y, int vec) {
    constexpr int NZ = 2 * RZ + 1, TZ = RZ ? 4 : 1, TY = RZ ? 64 : 256, PZ = TZ + 2 * RZ, PY = TY + 2, PX = MED_TX + 2, PLANE = PY * MED_PITCH, NC = 3 * NZ;
    static_assert(PZ * PLANE <= MED_FAST_LDS, "tile");
    __shared__ float tile[MED_FAST_LDS];
    const int tid = threadIdx.x;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % (unsigned)tiles_x) * MED_TX;
    b /= (unsigned)tiles_x;
    const int y0 = (int)(b % (unsigned)tiles_y) * TY, z0 = (int)(b / (unsigned)tiles_y) * TZ;
    const long long plane = (long long)H * W, image = (long long)blockIdx.y * D * plane;
    const float* img = src + image;
    for (int i = tid; i < PZ * PY * PX; i += 256) {
        const int c = i % PX, r = (i / PX) % PY, p = i / (PX * PY);
        const int gx = med_clamp(x0 - 1 + c, W), gy = med_clamp(y0 - 1 + r, H), gz = med_clamp(z0 - RZ + p, D);
        const float v = img[gz * plane + (long long)gy * W + gx];
        tile[p * PLANE + r * MED_PITCH + c] = !med_finite(v) ? NAN : v == 0.0f ? 0.0f : v;
    }
    __syncthreads();
    const int ly = RZ ? (tid & 63) : tid, lz = RZ ? (tid >> 6) : 0;
    const int y = y0 + ly, z = z0 + lz;
    if (y >= H || z >= D) return;
    const float* col = tile + lz * PLANE + ly * MED_PITCH;
    float* out = dst + image + z * plane + (long long)y * W;
    float c0[NC], c1[NC], c2[NC];
    bool bad0 = med_column<NZ, PLANE>(col, c0), bad1 = med_column<NZ, PLANE>(col + 1, c1);
#pragma unroll 1
    for (int xs = 0; xs < MED_TX; xs += 4) {
        const int gx = x0 + xs;
        if (gx >= W) break;
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool bad2 = med_column<NZ, PLANE>(col + xs + j + 2, c2);
            const float m = NZ == 3 ? med_select27(c0, c1, c2) : med_select9(c0, c1, c2);
            o[j] = (bad0 || bad1 || bad2) ? NAN : m;
#pragma unroll
            for (int k = 0; k < NC; ++k) { c0[k] = c1[k]; c1[k] = c2[k]; }
            bad0 = bad1; bad1 = bad2;
        }
        if (vec && gx + 4 <= W) {
            *reinterpret_cast<float4*>(out + gx) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (gx + j < W) out[gx + j] = o[j];
        }
    }
}

__device__ __forceinline__ unsigned med_key(float x) {      // unsigned order = float order; -0.0 and +0.0 share the key of +0.0; non-finite: MED_BAD_KEY
    if (!med_finite(x)) return MED_BAD_KEY;
    unsigned u = __float_as_uint(x);
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float med_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

struct MedGeneral {
    int D, H, W, rz, ry, rx;
    int la, lb;               // the workgroup's outputs: 2^la (x) * 2^lb (y) * 2^(8 - la - lb) (z)
    int tiles_x, tiles_y;
};

// grid (tiles_x * tiles_y * tiles_z, n), 256 threads; the staged tile has at most MED_GEN_LDS keys (checked by the host)
__global__ void __launch_bounds__(256) median_general_kernel(const float* __restrict__ src, float* __restrict__ dst, MedGeneral g) {
    __shared__ unsigned keys[MED_GEN_LDS];
    const int tid = threadIdx.x;
    const int tx = 1 << g.la, ty = 1 << g.lb, tz = 256 >> (g.la + g.lb);
    const int px = tx + 2 * g.rx, py = ty + 2 * g.ry, pz = tz + 2 * g.rz;
    unsigned b = blockIdx.x;
    const int x0 = (int)(b % (unsigned)g.tiles_x) * tx;
    b /= (unsigned)g.tiles_x;
    const int y0 = (int)(b % (unsigned)g.tiles_y) * ty, z0 = (int)(b / (unsigned)g.tiles_y) * tz;
    const long long plane = (long long)g.H * g.W, image = (long long)blockIdx.y * g.D * plane;
    const float* img = src + image;
    for (int i = tid; i < px * py * pz; i += 256) {
        const int c = i % px, r = (i / px) % py, p = i / (px * py);
        const int gx = med_clamp(x0 - g.rx + c, g.W), gy = med_clamp(y0 - g.ry + r, g.H), gz = med_clamp(z0 - g.rz + p, g.D);
        keys[i] = med_key(img[gz * plane + (long long)gy * g.W + gx]);
    }
    __syncthreads();
    const int lx = tid & (tx - 1), ly = (tid >> g.la) & (ty - 1), lz = tid >> (g.la + g.lb);
    const unsigned* win = keys + (lz * py + ly) * px + lx;
    const int nx = 2 * g.rx + 1, ny = 2 * g.ry + 1, nz = 2 * g.rz + 1;
    const unsigned k = (unsigned)(nx * ny * nz) / 2u;
    unsigned prefix = 0u, bad = 0u;
    for (int dz = 0; dz < nz; ++dz)
        for (int dy = 0; dy < ny; ++dy) {
            const unsigned* row = win + (dz * py + dy) * px;
            for (int dx = 0; dx < nx; ++dx) bad += row[dx] == MED_BAD_KEY;
        }
    for (int s = 30; s >= 0; s -= 2) {
        const unsigned t1 = prefix | (1u << s), t2 = prefix | (2u << s), t3 = prefix | (3u << s);
        unsigned n1 = 0u, n2 = 0u, n3 = 0u;
        for (int dz = 0; dz < nz; ++dz)
            for (int dy = 0; dy < ny; ++dy) {
                const unsigned* row = win + (dz * py + dy) * px;
                for (int dx = 0; dx < nx; ++dx) {
                    const unsigned key = row[dx];
                    n1 += key < t1; n2 += key < t2; n3 += key < t3;
                }
            }
        prefix = n3 <= k ? t3 : n2 <= k ? t2 : n1 <= k ? t1 : prefix;
    }
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x < g.W && y < g.H && z < g.D) dst[image + z * plane + (long long)y * g.W + x] = bad ? NAN : med_value(prefix);
}

}  // namespace mh
