// Overlap records for the segmentation metrics: DiceMetric / DiceHelper (monai/metrics/meandice.py:281-337), MeanIoU (meaniou.py:130-147) and
// ConfusionMatrixMetric (confusion_matrix.py:153-176) all reduce a prediction and a ground truth to a handful of sums per (batch item, class).  The
// reference forms them with a compare, a masked_select and three full-volume sums per class; here ONE pass over the two tensors leaves, for every
// (b, c), the eight fp64 sums below, and the metric classes finish on the [B, K]-sized record.
//
// For voxel i of (b, c): p, y = the fp32 values of prediction / truth for class c -- the stored value of a CHANNEL-form side [B][K][n], or
// (label == c) ? 1 : 0 of a LABEL-MAP side [B][1][n] (float32 / int64 labels truncated like .long(), uint8 as is; a label outside [0, K) is no class).
//   slot 0  sum of y where p != 0 (NaN counts as non-zero, like .bool())      slot 4  sum of p
//   slot 1  count of p != 0                                                    slot 5  count of (p + y) == 2   (fp32 add)
//   slot 2  sum of y                                                           slot 6  count of (p + y) == 0
//   slot 3  sum of y * p (fp32 product, fp64 accumulate)                       slot 7  count of p / y values that are neither 0 nor 1
//
// Streaming and HBM-bound by construction: a thread serves a CHUNK of up to 8 classes (unrolled, accumulators in registers under constant indices;
// gridDim.y walks the chunks) from one load of a label, so label x label reads both maps exactly once for K <= 8; channel x channel runs one class per
// chunk, so every row is read once as well.  16-byte loads over the part of a row where both sides are 16-byte aligned (rows of odd n are not: the
// head before it and the tail after it go element by element; rows whose two sides never line up go element by element throughout), a grid-stride
// loop over a grid sized from the CU count.  uint8 x uint8 label maps -- the fused-argmax output of the inferer against a stored segmentation -- count
// four voxels per 32-bit operation (zero-byte masks of word ^ class pattern, popcounts).
// Deterministic: no atomics.  Counts live in 32-bit lane counters and sums in fp64 (exact to 2^53; the headline volume's 2^27 voxels are past fp32's
// 2^24), waves fold with __shfl_xor butterflies, the four waves of a workgroup through LDS, every workgroup stores its record to
// workspace[b][block][K][8] and a one-wave kernel per (b, c) folds the blocks in a fixed order: the same input gives the same bits.
#pragma once
#include "common.h"

namespace mh {

enum { OV_CHANNEL = 0, OV_LABELS = 1 };
enum { OV_F32 = 0, OV_U8 = 1, OV_I64 = 2 };
enum { OV_SLOTS = 8, OV_CHUNK = 8, OV_MAX_BLOCKS = 2048 };

// class index of a label value: .long() truncation; what is no class index at all (negative, huge, NaN) is -1 and matches nothing
__device__ __forceinline__ int ov_class(float v) { return (v > -1.0f && v < 2.0e9f) ? (int)v : -1; }
__device__ __forceinline__ int ov_class(unsigned char v) { return (int)v; }
__device__ __forceinline__ int ov_class(long long v) { return (v >= 0 && v < 2000000000LL) ? (int)v : -1; }

// V consecutive elements from a 16-byte aligned address, as 16-byte loads
template <typename T, int V> __device__ __forceinline__ void ov_load(const T* __restrict__ p, T (&e)[V]) {
    constexpr int NL = V * (int)sizeof(T) / 16;
    uint4 raw[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) raw[j] = reinterpret_cast<const uint4*>(p)[j];
    __builtin_memcpy(e, raw, sizeof(raw));
}

// 0x80 in every byte of x that is zero, 0 elsewhere (exact: no carries between bytes)
__device__ __forceinline__ unsigned ov_zero_bytes(unsigned x) { return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); }

// the accumulators of one thread: label x label needs three counters per class (every slot follows from them and the voxel count)
template <bool BOTH> struct OvAcc;
template <> struct OvAcc<true> {
    unsigned cp[OV_CHUNK], cy[OV_CHUNK], cpy[OV_CHUNK], cnt;
};
template <> struct OvAcc<false> {
    double s0[OV_CHUNK], s2[OV_CHUNK], s3[OV_CHUNK], s4[OV_CHUNK];
    unsigned s1[OV_CHUNK], s5[OV_CHUNK], s6[OV_CHUNK], s7[OV_CHUNK];
};

template <int PF, int YF> __device__ __forceinline__ void ov_add(OvAcc<false>& a, const int k, const float p, const float y) {
    const bool pn = p != 0.0f;                       // NaN != 0
    a.s0[k] += pn ? (double)y : 0.0;
    a.s1[k] += pn ? 1u : 0u;
    a.s2[k] += (double)y;
    a.s3[k] += (double)(y * p);
    a.s4[k] += (double)p;
    const float t = p + y;
    a.s5[k] += t == 2.0f ? 1u : 0u;
    a.s6[k] += t == 0.0f ? 1u : 0u;
    if (PF == OV_CHANNEL) a.s7[k] += (p != 0.0f && p != 1.0f) ? 1u : 0u;
    if (YF == OV_CHANNEL) a.s7[k] += (y != 0.0f && y != 1.0f) ? 1u : 0u;
}

// One voxel at offset i of the rows, every class of the chunk.  prow / yrow: the label row of a label-map side, the row of class c0 of a channel side.
template <int PF, typename TP, int YF, typename TY, int CH>
__device__ __forceinline__ void ov_voxel(OvAcc<PF == OV_LABELS && YF == OV_LABELS>& a, const TP* __restrict__ prow, const TY* __restrict__ yrow, const long long i,
                                         const long long n, const int c0, const int nc) {
    constexpr bool BOTH = PF == OV_LABELS && YF == OV_LABELS;
    const int lp = PF == OV_LABELS ? ov_class(prow[i]) : 0, ly = YF == OV_LABELS ? ov_class(yrow[i]) : 0;
    if constexpr (BOTH) a.cnt += 1u;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        if (k < nc) {
            if constexpr (BOTH) {
                const bool bp = lp == c0 + k, by = ly == c0 + k;
                a.cp[k] += bp ? 1u : 0u;
                a.cy[k] += by ? 1u : 0u;
                a.cpy[k] += (bp && by) ? 1u : 0u;
            } else {
                const float p = PF == OV_LABELS ? (lp == c0 + k ? 1.0f : 0.0f) : (float)prow[(long long)k * n + i];
                const float y = YF == OV_LABELS ? (ly == c0 + k ? 1.0f : 0.0f) : (float)yrow[(long long)k * n + i];
                ov_add<PF, YF>(a, k, p, y);
            }
        }
    }
}

// grid (blocks, class chunks of CH, B); workspace [B][gridDim.x][K][8]
template <int PF, typename TP, int YF, typename TY, int CH>
__global__ void __launch_bounds__(256) overlap_partial_kernel(const TP* __restrict__ pred, const TY* __restrict__ truth, int K, long long n,
                                                              double* __restrict__ workspace) {
    constexpr bool BOTH = PF == OV_LABELS && YF == OV_LABELS;
    constexpr int VP = 16 / (int)sizeof(TP), VY = 16 / (int)sizeof(TY), V = VP > VY ? VP : VY;
    const int b = blockIdx.z, c0 = blockIdx.y * CH, nc = (K - c0) < CH ? (K - c0) : CH;
    const TP* __restrict__ prow = pred + (PF == OV_LABELS ? (long long)b * n : ((long long)b * K + c0) * n);
    const TY* __restrict__ yrow = truth + (YF == OV_LABELS ? (long long)b * n : ((long long)b * K + c0) * n);

    // [head, head + nvec * V): the part of the rows that both sides (and every class row of a channel side) can read with 16-byte loads
    const long long mis_p = (long long)((reinterpret_cast<uintptr_t>(prow) & 15u) / sizeof(TP)), mis_y = (long long)((reinterpret_cast<uintptr_t>(yrow) & 15u) / sizeof(TY));
    long long head = VP >= VY ? (V - mis_p) % V : (V - mis_y) % V;
    bool vec = (head + mis_p) % VP == 0 && (head + mis_y) % VY == 0;
    if (PF == OV_CHANNEL && nc > 1 && n % VP != 0) vec = false;      // the rows of the other classes start n elements on
    if (YF == OV_CHANNEL && nc > 1 && n % VY != 0) vec = false;
    if (!vec || head > n) head = n;
    const long long nvec = (n - head) / V, tail0 = head + nvec * V;

    OvAcc<BOTH> a = {};
    const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long i = t0; i < head; i += step) ov_voxel<PF, TP, YF, TY, CH>(a, prow, yrow, i, n, c0, nc);
    for (long long i = tail0 + t0; i < n; i += step) ov_voxel<PF, TP, YF, TY, CH>(a, prow, yrow, i, n, c0, nc);
    for (long long g = t0; g < nvec; g += step) {
        const long long i = head + g * V;
        if constexpr (BOTH && sizeof(TP) == 1 && sizeof(TY) == 1) {
            // uint8 x uint8 label maps: four voxels per 32-bit word
            unsigned char ep[V], ey[V];
            ov_load<TP, V>(prow + i, ep);
            ov_load<TY, V>(yrow + i, ey);
            unsigned wp[4], wy[4];
            __builtin_memcpy(wp, ep, 16);
            __builtin_memcpy(wy, ey, 16);
            a.cnt += (unsigned)V;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (k < nc && c0 + k < 256) {
                    const unsigned pat = (unsigned)(c0 + k) * 0x01010101u;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned zp = ov_zero_bytes(wp[j] ^ pat), zy = ov_zero_bytes(wy[j] ^ pat);
                        a.cp[k] += (unsigned)__builtin_popcount(zp);
                        a.cy[k] += (unsigned)__builtin_popcount(zy);
                        a.cpy[k] += (unsigned)__builtin_popcount(zp & zy);
                    }
                }
            }
        } else {
            int lp[V], ly[V];
            if constexpr (PF == OV_LABELS) {
                TP e[V];
                ov_load<TP, V>(prow + i, e);
#pragma unroll
                for (int j = 0; j < V; ++j) lp[j] = ov_class(e[j]);
            }
            if constexpr (YF == OV_LABELS) {
                TY e[V];
                ov_load<TY, V>(yrow + i, e);
#pragma unroll
                for (int j = 0; j < V; ++j) ly[j] = ov_class(e[j]);
            }
            if constexpr (BOTH) a.cnt += (unsigned)V;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (k < nc) {
                    if constexpr (BOTH) {
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            const bool bp = lp[j] == c0 + k, by = ly[j] == c0 + k;
                            a.cp[k] += bp ? 1u : 0u;
                            a.cy[k] += by ? 1u : 0u;
                            a.cpy[k] += (bp && by) ? 1u : 0u;
                        }
                    } else {
                        TP ep[V];
                        TY ey[V];
                        if constexpr (PF == OV_CHANNEL) ov_load<TP, V>(prow + (long long)k * n + i, ep);
                        if constexpr (YF == OV_CHANNEL) ov_load<TY, V>(yrow + (long long)k * n + i, ey);
#pragma unroll
                        for (int j = 0; j < V; ++j) {
                            float p, y;
                            if constexpr (PF == OV_LABELS) p = lp[j] == c0 + k ? 1.0f : 0.0f; else p = (float)ep[j];
                            if constexpr (YF == OV_LABELS) y = ly[j] == c0 + k ? 1.0f : 0.0f; else y = (float)ey[j];
                            ov_add<PF, YF>(a, k, p, y);
                        }
                    }
                }
            }
        }
    }

    // lanes -> wave (butterflies) -> workgroup (LDS, waves added in order) -> this block's record
    constexpr int NR = BOTH ? 4 : OV_SLOTS;
    __shared__ double red[4][CH][NR];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        if (k < nc) {
            double v[NR];
            if constexpr (BOTH) {
                v[0] = (double)a.cpy[k]; v[1] = (double)a.cp[k]; v[2] = (double)a.cy[k]; v[3] = (double)a.cnt;
            } else {
                v[0] = a.s0[k]; v[1] = (double)a.s1[k]; v[2] = a.s2[k]; v[3] = a.s3[k];
                v[4] = a.s4[k]; v[5] = (double)a.s5[k]; v[6] = (double)a.s6[k]; v[7] = (double)a.s7[k];
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v[r] += __shfl_xor(v[r], o);
                if (lane == 0) red[wave][k][r] = v[r];
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nc * OV_SLOTS) {
        const int k = threadIdx.x >> 3, s = threadIdx.x & 7;
        double r;
        if constexpr (BOTH) {
            const double py = red[0][k][0] + red[1][k][0] + red[2][k][0] + red[3][k][0], p = red[0][k][1] + red[1][k][1] + red[2][k][1] + red[3][k][1];
            const double y = red[0][k][2] + red[1][k][2] + red[2][k][2] + red[3][k][2], cnt = red[0][k][3] + red[1][k][3] + red[2][k][3] + red[3][k][3];
            r = (s == 0 || s == 3 || s == 5) ? py : (s == 1 || s == 4) ? p : s == 2 ? y : s == 6 ? cnt - p - y + py : 0.0;
        } else {
            r = red[0][k][s] + red[1][k][s] + red[2][k][s] + red[3][k][s];
        }
        workspace[((((long long)b * gridDim.x + blockIdx.x) * K) + c0 + k) * OV_SLOTS + s] = r;
    }
}

// one wave per (c, b): the records of the blocks, lane i taking blocks i, i + 64, ... in order, then a butterfly -- a fixed summation tree
__global__ void __launch_bounds__(64) overlap_final_kernel(const double* __restrict__ workspace, int nblocks, int K, double* __restrict__ out) {
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    double a[OV_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < nblocks; i += 64) {
        const double* r = workspace + (((long long)b * nblocks + i) * K + c) * OV_SLOTS;
#pragma unroll
        for (int s = 0; s < OV_SLOTS; ++s) a[s] += r[s];
    }
#pragma unroll
    for (int s = 0; s < OV_SLOTS; ++s) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a[s] += __shfl_xor(a[s], o);
    }
    if (lane == 0) {
        double* o = out + ((long long)b * K + c) * OV_SLOTS;
#pragma unroll
        for (int s = 0; s < OV_SLOTS; ++s) o[s] = a[s];
    }
}

}  // namespace mh
