// Surface metrics: HausdorffDistanceMetric (monai/metrics/hausdorff_distance.py:132-212), SurfaceDistanceMetric (surface_distance.py:123-186) and
// SurfaceDiceMetric (surface_dice.py:137-279) all reduce, per (batch item, class), the distances from the edge voxels of one mask to the nearest edge
// voxel of the other.  The reference walks the (b, c) pairs in Python and runs scipy's binary_erosion and distance_transform_edt on the host for each
// (metrics/utils.py:139-344); the exact Euclidean distance transform is also public on its own (monai/transforms/utils.py distance_transform_edt,
// DistanceTransformEDT).  Here every kernel is batched over a leading ITEM index (blockIdx.y): one launch serves every batch item, class and direction.
//
//   surf_bbox_*      per (b, c): bounding box of pred | truth with margin 1, clipped to the volume, and whether each side has any foreground
//   surf_edge_kernel mask & ~erode(mask) over a box: face-connected element (2 * rank neighbours), outside the volume = background
//   edt_row_kernel   pass 1 along the contiguous axis: one wave per row, prefix-max / suffix-min of the feature index with wave shuffles
//   edt_col_kernel   one pass per remaining axis: lower envelope of parabolas (Meijster, Roerdink, Hesselink 2000) per column, one thread per
//                    column, lanes across the contiguous axis (every load and store coalesced), stack in a workspace laid out [k][column]
//   edt_finish_kernel sqrt in fp64, stored as fp64 or rounded once to fp32
//   surf_partial_kernel / surf_final_kernel  per item: count of source edge voxels, max squared distance, fp64 sum of the fp32 distances, count of
//                    (float)d <= (float)threshold; with `write` the compacted fp32 distances in voxel order.  No atomics: fixed summation trees.
//
// Squared distances: unit spacing int32, exact (3 * 2048^2 < 2^31: axes up to 2048), the parabola intersection in integer arithmetic; with a
// spacing the same structure in fp64.  A row / column without a feature carries a SENTINEL (INT_MAX / +inf), never a large finite number; an item
// without any feature comes out +inf everywhere.
#pragma once
#include "common.h"
#include "metrics.h"

namespace mh {

enum { ED_BOOL = 3, ED_MAX_AXIS = 2048, ED_BOX_BLOCKS = 64, ED_REC_BLOCKS = 256, ED_REC_SLOTS = 4 };

// one row of an item table (16 x 8 bytes, built on the host): which fields a kernel reads is said at the kernel
struct EdItem {
    long long off;            // voxel offset of the item's box in the per-call buffers (edge map, fields, stack)
    long long d, h, w;        // box extent
    double sz, sy, sx;        // spacing
    long long b, c;           // batch item, class
    long long z0, y0, x0;     // box origin in the volume
    long long src_off;        // records: offset of the source edge map
    long long fld_off;        // records: offset of the squared-distance field of the other side's edges
    double thr;               // records: threshold (a float32 value)
    long long out_off;        // records, write: offset of the item's compacted distances
};

template <typename V> struct EdVal;
template <> struct EdVal<int> {
    static __device__ __forceinline__ int sent() { return 0x7fffffff; }
    static __device__ __forceinline__ bool is_sent(int v) { return v == 0x7fffffff; }
    static __device__ __forceinline__ int sq(int g, double) { return g * g; }
    static __device__ __forceinline__ double dist(int v) { return v == 0x7fffffff ? __builtin_huge_val() : sqrt((double)v); }
    static __device__ __forceinline__ double as_double(int v) { return v == 0x7fffffff ? __builtin_huge_val() : (double)v; }
};
template <> struct EdVal<double> {
    static __device__ __forceinline__ double sent() { return __builtin_huge_val(); }
    static __device__ __forceinline__ bool is_sent(double v) { return v == __builtin_huge_val(); }
    static __device__ __forceinline__ double sq(int g, double sp) { const double t = (double)g * sp; return t * t; }
    static __device__ __forceinline__ double dist(double v) { return sqrt(v); }
    static __device__ __forceinline__ double as_double(double v) { return v; }
};

// foreground of class c at voxel i of batch item b: a bool channel as it is, another channel value == 1, a label == c
template <int FORM, typename T, bool ISBOOL>
__device__ __forceinline__ bool ed_fg(const T* __restrict__ src, int K, long long n, int b, int c, long long i) {
    if (FORM == OV_CHANNEL) {
        const T v = src[((long long)b * K + c) * n + i];
        return ISBOOL ? (v != (T)0) : (v == (T)1);
    }
    return ov_class(src[(long long)b * n + i]) == c;
}

// ---------------------------------------------------------------------------------------------------------------- boxes
// grid (ED_BOX_BLOCKS, nc, B); workspace int32 [B][nc][2 sides][gridDim.x][8]: zmin ymin xmin zmax ymax xmax any -
template <int FORM, typename T, bool ISBOOL>
__global__ void __launch_bounds__(256) surf_bbox_partial_kernel(const T* __restrict__ src, int K, int c0, int D, int H, int W, int side, int* __restrict__ ws) {
    const int b = blockIdx.z, ci = blockIdx.y, c = c0 + ci;
    const long long n = (long long)D * H * W, hw = (long long)H * W;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (ed_fg<FORM, T, ISBOOL>(src, K, n, b, c, i)) {
            const int z = (int)(i / hw), r = (int)(i - (long long)z * hw), y = r / W, x = r - y * W;
            lo[0] = min(lo[0], z); lo[1] = min(lo[1], y); lo[2] = min(lo[2], x);
            hi[0] = max(hi[0], z); hi[1] = max(hi[1], y); hi[2] = max(hi[2], x);
        }
    }
    __shared__ int red[4][6];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], __shfl_xor(lo[a], o));
            hi[a] = max(hi[a], __shfl_xor(hi[a], o));
        }
        if (lane == 0) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int s = threadIdx.x;
        int v = 0;
        if (s < 3) v = min(min(red[0][s], red[1][s]), min(red[2][s], red[3][s]));
        else if (s < 6) v = max(max(red[0][s], red[1][s]), max(red[2][s], red[3][s]));
        else if (s == 6) v = max(max(red[0][3], red[1][3]), max(red[2][3], red[3][3])) >= 0 ? 1 : 0;
        ws[(((((long long)b * gridDim.y + ci) * 2 + side) * gridDim.x) + blockIdx.x) * 8 + s] = v;
    }
}

// grid (P = B * nc), one wave; boxes int32 [P][8]: z0 y0 x0 d h w has_pred has_truth (margin 1, clipped; d = h = w = 0 without foreground)
__global__ void __launch_bounds__(64) surf_bbox_final_kernel(const int* __restrict__ ws, int nblk, int D, int H, int W, int* __restrict__ boxes) {
    const int p = blockIdx.x, lane = threadIdx.x;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1}, any[2] = {0, 0};
    for (int i = lane; i < 2 * nblk; i += 64) {
        const int* r = ws + ((long long)p * 2 * nblk + i) * 8;
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], r[a]); hi[a] = max(hi[a], r[3 + a]); }
        any[i / nblk] |= r[6];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], __shfl_xor(lo[a], o)); hi[a] = max(hi[a], __shfl_xor(hi[a], o)); }
        any[0] = max(any[0], __shfl_xor(any[0], o));
        any[1] = max(any[1], __shfl_xor(any[1], o));
    }
    if (lane == 0) {
        int* o = boxes + (long long)p * 8;
        const int ext[3] = {D, H, W};
        if (hi[0] < 0) {
            for (int a = 0; a < 6; ++a) o[a] = 0;
        } else {
            for (int a = 0; a < 3; ++a) {
                const int s = max(lo[a] - 1, 0), e = min(hi[a] + 1, ext[a] - 1);
                o[a] = s; o[3 + a] = e - s + 1;
            }
        }
        o[6] = any[0]; o[7] = any[1];
    }
}

// ---------------------------------------------------------------------------------------------------------------- edges
// grid (blocks, items); item: off, d h w, b c, z0 y0 x0.  rank = spatial rank of the volume (leading extents of a lower rank are 1 and no neighbour axis)
template <int FORM, typename T, bool ISBOOL>
__global__ void __launch_bounds__(256) surf_edge_kernel(const T* __restrict__ src, int K, int rank, int D, int H, int W, const EdItem* __restrict__ items,
                                                         unsigned char* __restrict__ edges) {
    const EdItem it = items[blockIdx.y];
    const int bd = (int)it.d, bh = (int)it.h, bw = (int)it.w, b = (int)it.b, c = (int)it.c;
    const long long nvox = (long long)bd * bh * bw, n = (long long)D * H * W, hw = (long long)H * W;
    const int ext[3] = {D, H, W};
    const long long str[3] = {hw, (long long)W, 1LL};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        const int bz = (int)(i / ((long long)bh * bw)), r = (int)(i - (long long)bz * bh * bw), by = r / bw, bx = r - by * bw;
        const int p[3] = {bz + (int)it.z0, by + (int)it.y0, bx + (int)it.x0};
        const long long v = (long long)p[0] * hw + (long long)p[1] * W + p[2];
        bool edge = false;
        if (ed_fg<FORM, T, ISBOOL>(src, K, n, b, c, v)) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (a >= 3 - rank) {
                    if (p[a] == 0 || !ed_fg<FORM, T, ISBOOL>(src, K, n, b, c, v - str[a])) edge = true;
                    if (p[a] == ext[a] - 1 || !ed_fg<FORM, T, ISBOOL>(src, K, n, b, c, v + str[a])) edge = true;
                }
            }
        }
        edges[it.off + i] = edge ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- EDT
// Pass 1, grid (ceil(max rows / 4), items), 256 threads = 4 waves = 4 rows; item: off, d h w, sx.  A feature is a map value != 0 (== 0 with `invert`).
// out = squared distance along the row to the nearest feature of the row, or the sentinel.  `out` doubles as the store of the forward sweep.
template <typename T, typename V>
__global__ void __launch_bounds__(256) edt_row_kernel(const T* __restrict__ map, int invert, const EdItem* __restrict__ items, V* __restrict__ out) {
    const EdItem it = items[blockIdx.y];
    const int w = (int)it.w, lane = threadIdx.x & 63;
    const long long rows = it.d * it.h, row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                  // a whole wave leaves; the kernel has no workgroup barrier
    const long long base = it.off + row * w;
    const int chunks = (w + 63) / 64;
    int carry = -1;                                           // index of the nearest feature at or before x
    for (int ch = 0; ch < chunks; ++ch) {
        const int x = ch * 64 + lane;
        int v = (x < w && ((map[base + x] != (T)0) != (invert != 0))) ? x : -1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl(v, lane >= o ? lane - o : lane);
            if (lane >= o) v = max(v, t);
        }
        v = max(v, carry);
        carry = __shfl(v, 63);
        if (x < w) out[base + x] = v < 0 ? EdVal<V>::sent() : (V)(x - v);
    }
    const int none = 0x7fffffff;
    carry = none;                                             // index of the nearest feature at or after x
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int x = ch * 64 + lane;
        int v = (x < w && ((map[base + x] != (T)0) != (invert != 0))) ? x : none;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl(v, lane + o < 64 ? lane + o : lane);
            if (lane + o < 64) v = min(v, t);
        }
        v = min(v, carry);
        carry = __shfl(v, 0);
        if (x < w) {
            const V left = out[base + x];
            int g = EdVal<V>::is_sent(left) ? -1 : (int)left;
            if (v != none) g = g < 0 ? v - x : min(g, v - x);
            out[base + x] = g < 0 ? EdVal<V>::sent() : EdVal<V>::sq(g, it.sx);
        }
    }
}

// value at x of the parabola rooted at i with height f
__device__ __forceinline__ int ed_F(int x, int i, int f, double) { return (x - i) * (x - i) + f; }
__device__ __forceinline__ double ed_F(int x, int i, double f, double sp) { const double t = (double)(x - i) * sp; return t * t + f; }
// first integer position from which parabola u (> s) is the lower one, as a double where the arithmetic is (may be huge); s's region is never left empty
__device__ __forceinline__ int ed_next(int s, int u, int fs, int fu, double, int t, int n) {
    const int num = u * u - s * s + fu - fs;                  // >= 0 after the pops; < 2^31: u^2 <= 2^22, f <= 3 * 2^22
    return 1 + num / (2 * (u - s));
}
__device__ __forceinline__ int ed_next(int s, int u, double fs, double fu, double sp, int t, int n) {
    const double sp2 = sp * sp, x = (fu - fs + sp2 * (double)(u * u - s * s)) / (2.0 * sp2 * (double)(u - s));
    const double wd = floor(x) + 1.0;
    if (!(wd < (double)n)) return n;
    const int w = (int)wd;
    return w > t ? w : t + 1;
}

// Pass 2 / 3, grid (ceil(max columns / 256), items); item: off, d h w, sz sy.  axis 1: columns along y of (z, x); axis 0: columns along z of (y, x).
// in -> out (different buffers: the backward sweep reads heights the forward sweep left behind); stack uint32 [k][column] = root | first position << 16
template <typename V>
__global__ void __launch_bounds__(256) edt_col_kernel(const V* __restrict__ in, V* __restrict__ out, unsigned* __restrict__ stack, const EdItem* __restrict__ items,
                                                       int axis) {
    const EdItem it = items[blockIdx.y];
    const long long hw = it.h * it.w, ncols = axis == 1 ? it.d * it.w : hw, col = (long long)blockIdx.x * 256 + threadIdx.x;
    if (col >= ncols) return;
    const int n = axis == 1 ? (int)it.h : (int)it.d;
    const long long stride = axis == 1 ? it.w : hw, base = it.off + (axis == 1 ? (col / it.w) * hw + col % it.w : col);
    const double sp = axis == 1 ? it.sy : it.sz;
    unsigned* __restrict__ stk = stack + it.off + col;
    int q = -1, s = 0, t = 0;
    V fs = 0;
    for (int u = 0; u < n; ++u) {
        const V fu = in[base + u * stride];
        if (EdVal<V>::is_sent(fu)) continue;
        while (q >= 0 && ed_F(t, s, fs, sp) > ed_F(t, u, fu, sp)) {
            --q;
            if (q >= 0) {
                const unsigned e = stk[q * ncols];
                s = (int)(e & 0xffffu); t = (int)(e >> 16); fs = in[base + s * stride];
            }
        }
        if (q < 0) {
            q = 0; s = u; t = 0; fs = fu;
            stk[0] = (unsigned)u;
        } else {
            const int wn = ed_next(s, u, fs, fu, sp, t, n);
            if (wn < n) {
                ++q; s = u; t = wn; fs = fu;
                stk[q * ncols] = (unsigned)u | ((unsigned)wn << 16);
            }
        }
    }
    if (q < 0) {
        for (int u = 0; u < n; ++u) out[base + u * stride] = EdVal<V>::sent();
        return;
    }
    for (int u = n - 1; u >= 0; --u) {
        while (t > u) {
            --q;
            const unsigned e = stk[q * ncols];
            s = (int)(e & 0xffffu); t = (int)(e >> 16); fs = in[base + s * stride];
        }
        out[base + u * stride] = ed_F(u, s, fs, sp);
    }
}

// sqrt in fp64, stored as OUT; grid-stride over all voxels of the call
template <typename V, typename OUT>
__global__ void __launch_bounds__(256) edt_finish_kernel(const V* __restrict__ field, long long total, OUT* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) out[i] = (OUT)EdVal<V>::dist(field[i]);
}

// ---------------------------------------------------------------------------------------------------------------- records
// grid (nblk, items), 256 threads; item: d * h * w voxels, src_off, fld_off, thr, out_off.  Block k serves the k-th contiguous piece of the item (pieces of
// whole 256-voxel trips), so the pieces' counts give every block its place in the compacted output.  ws double [item][nblk][4].
// write = 0: the four partial values to ws.  write = 1: ws (of the write = 0 call) is read, the fp32 distances go to dist[out_off + rank in voxel order].
template <typename V>
__global__ void __launch_bounds__(256) surf_partial_kernel(const unsigned char* __restrict__ edges, const V* __restrict__ field, const EdItem* __restrict__ items,
                                                            int write, double* __restrict__ ws, float* __restrict__ dist, long long ndist) {
    const EdItem it = items[blockIdx.y];
    const long long nvox = it.d * it.h * it.w;
    long long piece = (nvox + gridDim.x - 1) / gridDim.x;
    piece = (piece + 255) / 256 * 256;
    const long long start = (long long)blockIdx.x * piece, end = min(nvox, start + piece);
    const float thr = (float)it.thr;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ double red[4][ED_REC_SLOTS];
    __shared__ long long place;
    __shared__ int wtot[4];
    if (write) {
        if (threadIdx.x == 0) {
            double before = 0.0;
            for (unsigned k = 0; k < blockIdx.x; ++k) before += ws[((long long)blockIdx.y * gridDim.x + k) * ED_REC_SLOTS];
            place = it.out_off + (long long)before;
        }
        __syncthreads();
    }
    long long at = write ? place : 0;
    unsigned cnt = 0, cthr = 0;
    double sum = 0.0, mx = -1.0;
    for (long long pos = start; pos < end; pos += 256) {              // the same trips for every thread of the block
        const long long i = pos + threadIdx.x;
        const bool on = i < end && edges[it.src_off + i] != 0;
        float d = 0.0f;
        if (on) {
            const V f = field[it.fld_off + i];
            d = (float)EdVal<V>::dist(f);
            cnt += 1u;
            sum += (double)d;
            mx = fmax(mx, EdVal<V>::as_double(f));
            cthr += d <= thr ? 1u : 0u;
        }
        if (write) {
            int v = on ? 1 : 0;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl(v, lane >= o ? lane - o : lane);
                if (lane >= o) v += t;
            }
            if (lane == 63) wtot[wave] = v;
            __syncthreads();
            int before = 0;
            for (int k = 0; k < wave; ++k) before += wtot[k];
            if (on && at + before + v - 1 < ndist) dist[at + before + v - 1] = d;      // the bound only guards a caller whose offsets do not match the counts
            at += wtot[0] + wtot[1] + wtot[2] + wtot[3];
            __syncthreads();
        }
    }
    if (write) return;
    double v[ED_REC_SLOTS] = {(double)cnt, mx, sum, (double)cthr};
#pragma unroll
    for (int r = 0; r < ED_REC_SLOTS; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_xor(v[r], o);
            v[r] = r == 1 ? fmax(v[r], t) : v[r] + t;
        }
        if (lane == 0) red[wave][r] = v[r];
    }
    __syncthreads();
    if (threadIdx.x < ED_REC_SLOTS) {
        const int r = threadIdx.x;
        const double a = r == 1 ? fmax(fmax(red[0][r], red[1][r]), fmax(red[2][r], red[3][r])) : red[0][r] + red[1][r] + red[2][r] + red[3][r];
        ws[((long long)blockIdx.y * gridDim.x + blockIdx.x) * ED_REC_SLOTS + r] = a;
    }
}

// one wave per item: lane i folds blocks i, i + 64, ... in order, then a butterfly.  out double [item][4]: count, max squared distance (-1 without an
// edge voxel, +inf where the field holds the sentinel), sum of the fp32 distances, count within the threshold
__global__ void __launch_bounds__(64) surf_final_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ out) {
    const int item = blockIdx.x, lane = threadIdx.x;
    double a[ED_REC_SLOTS] = {0.0, -1.0, 0.0, 0.0};
    for (int i = lane; i < nblk; i += 64) {
        const double* r = ws + ((long long)item * nblk + i) * ED_REC_SLOTS;
        a[0] += r[0]; a[1] = fmax(a[1], r[1]); a[2] += r[2]; a[3] += r[3];
    }
#pragma unroll
    for (int r = 0; r < ED_REC_SLOTS; ++r) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double t = __shfl_xor(a[r], o);
            a[r] = r == 1 ? fmax(a[r], t) : a[r] + t;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < ED_REC_SLOTS; ++r) out[(long long)item * ED_REC_SLOTS + r] = a[r];
    }
}

}  // namespace mh
