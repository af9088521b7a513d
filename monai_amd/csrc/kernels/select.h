// Exact order statistics of a batch of fp32 runs: the selection primitive behind ScaleIntensityRangePercentiles and ClipIntensityPercentiles
// (monai/transforms/intensity/array.py:1299-1418, 1015-1157 -> percentile(), monai/transforms/utils_pytorch_numpy_unification.py:104-136: a host copy plus
// np.percentile above 1,000,000 elements, a full torch.quantile sort below).  Input: C runs of n contiguous values (blockIdx.y = run); at most SEL_MAX_RANKS
// ranks per run, the same for every run.  Radix select over order-preserving 32-bit keys, 11 + 11 + 10 bits:
//
//   select_count_kernel<PASS>   reads the runs once.  Pass 0 counts the top 11 key bits of every value (and the NaNs); passes 1 and 2 count the next digit of the
//                               keys that carry a LIVE prefix -- one prefix per rank, equal prefixes share a slot (the ranks k, k + 1 of one percentile nearly
//                               always do).  A workgroup counts into LDS (<= 4 slots x 2048 bins) and adds its non-zero bins to the run's histogram with
//                               integer atomics: sums of integers, the same bits whatever the order
//   select_scan_kernel<PASS>    one workgroup per run: the bin in which each rank falls (an exclusive scan over the slot's bins), the rank's new prefix and
//                               what remains of the rank inside it, the slots of the next pass; after pass 2 the prefix IS the key: the value goes out
//   percentile_lerp_kernel      one thread per (run, percentile): the interpolation between two order statistics in the reference's arithmetic
//
// Nothing comes back to the host between the passes: prefixes, remaining ranks and slots live in SelState words in device memory.
// Keys: -0.0 and +0.0 share the key of +0.0 (they compare equal in the reference's sorts; a selected zero is +0.0), +-inf are ordinary keys, a run that holds
// a NaN yields NaN for every rank (np.percentile and torch.quantile both do).  n < 2^31 per run: every count fits an unsigned word.
#pragma once
#include "common.h"

namespace mh {

enum { SEL_MAX_RANKS = 4, SEL_BINS = 2048, SEL_LERP_TORCH = 0, SEL_LERP_NUMPY = 1 };

struct SelState {                          // per run, 16 words, zeroed together with the histograms
    unsigned nan;                          // NaNs seen by pass 0
    unsigned nslots;                       // distinct live prefixes
    unsigned slot_prefix[SEL_MAX_RANKS];
    unsigned slot_of[SEL_MAX_RANKS];       // rank -> slot
    unsigned rem[SEL_MAX_RANKS];           // the rank's position among the keys of its prefix
    unsigned spare[2];
};
struct SelRanks { unsigned k[SEL_MAX_RANKS]; int R; };
struct SelLerp { double w[SEL_MAX_RANKS / 2]; int P, mode; };

#ifdef MH_SIMT_EMULATOR
// the fibers of one workgroup share a host thread (LDS: a plain add); workgroups run on several host threads (global memory: the compiler's builtin)
__device__ __forceinline__ void sel_add_lds(unsigned* p, unsigned v) { *p += v; }
__device__ __forceinline__ void sel_add_global(unsigned* p, unsigned v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ void sel_add_lds(unsigned* p, unsigned v) { atomicAdd(p, v); }
__device__ __forceinline__ void sel_add_global(unsigned* p, unsigned v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

__device__ __forceinline__ unsigned sel_key(float x) {
    unsigned u = __float_as_uint(x);
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

template <int PASS>
__device__ __forceinline__ void sel_count_one(float x, unsigned (*h)[SEL_BINS], const unsigned* pf, int ns, unsigned& nan) {
    const unsigned key = sel_key(x);
    if (PASS == 0) {
        nan += x != x ? 1u : 0u;
        sel_add_lds(&h[0][key >> 21], 1u);
    } else {
        const unsigned p = PASS == 1 ? key >> 21 : key >> 10, d = PASS == 1 ? (key >> 10) & 2047u : key & 1023u;
#pragma unroll
        for (int s = 0; s < SEL_MAX_RANKS; ++s)
            if (s < ns && p == pf[s]) sel_add_lds(&h[s][d], 1u);
    }
}

// grid (parts, C), 256 threads; hist: this pass's [C][SEL_MAX_RANKS][SEL_BINS] words.  VEC: the run starts 16-byte aligned; the n % 4 last values go one by one
template <int PASS, bool VEC>
__global__ void __launch_bounds__(256) select_count_kernel(const float* __restrict__ src, long long n, unsigned* __restrict__ hist, SelState* __restrict__ state) {
    __shared__ unsigned h[PASS == 0 ? 1 : SEL_MAX_RANKS][SEL_BINS];
    __shared__ unsigned nan_s;
    const int c = blockIdx.y, tid = threadIdx.x;
    const int ns = PASS == 0 ? 1 : (int)state[c].nslots;
    unsigned pf[SEL_MAX_RANKS];
#pragma unroll
    for (int s = 0; s < SEL_MAX_RANKS; ++s) pf[s] = (PASS != 0 && s < ns) ? state[c].slot_prefix[s] : 0xffffffffu;      // a prefix has at most 22 bits
    for (int s = 0; s < ns; ++s)
        for (int b = tid; b < SEL_BINS; b += 256) h[s][b] = 0u;
    if (tid == 0) nan_s = 0u;
    __syncthreads();
    const float* p = src + (long long)c * n;
    unsigned nan = 0u;
    const long long t0 = (long long)blockIdx.x * 256 + tid, step = (long long)gridDim.x * 256;
    if (VEC) {
        const long long n4 = n / 4;
        for (long long i = t0; i < n4; i += step) {
            const float4 v = *reinterpret_cast<const float4*>(p + 4 * i);
            sel_count_one<PASS>(v.x, h, pf, ns, nan); sel_count_one<PASS>(v.y, h, pf, ns, nan);
            sel_count_one<PASS>(v.z, h, pf, ns, nan); sel_count_one<PASS>(v.w, h, pf, ns, nan);
        }
        if (blockIdx.x == 0 && 4 * n4 + tid < n) sel_count_one<PASS>(p[4 * n4 + tid], h, pf, ns, nan);
    } else {
        for (long long i = t0; i < n; i += step) sel_count_one<PASS>(p[i], h, pf, ns, nan);
    }
    if (PASS == 0 && nan) sel_add_lds(&nan_s, nan);
    __syncthreads();
    unsigned* g = hist + (long long)c * SEL_MAX_RANKS * SEL_BINS;
    for (int s = 0; s < ns; ++s)
        for (int b = tid; b < SEL_BINS; b += 256) {
            const unsigned v = h[s][b];
            if (v) sel_add_global(g + s * SEL_BINS + b, v);
        }
    if (PASS == 0 && tid == 0 && nan_s) sel_add_global(&state[c].nan, nan_s);
}

// grid C, 256 threads, 8 consecutive bins per thread.  PASS 2 writes out[c][r] (r < R)
template <int PASS>
__global__ void __launch_bounds__(256) select_scan_kernel(const unsigned* __restrict__ hist, SelState* __restrict__ state, SelRanks rk, float* __restrict__ out) {
    __shared__ unsigned part[SEL_MAX_RANKS][256];
    __shared__ unsigned newp[SEL_MAX_RANKS], newrem[SEL_MAX_RANKS];
    const int c = blockIdx.x, t = threadIdx.x;
    SelState& st = state[c];
    const unsigned* g = hist + (long long)c * SEL_MAX_RANKS * SEL_BINS;
    const int ns = PASS == 0 ? 1 : (int)st.nslots;
    const int bits = PASS == 2 ? 10 : 11;
    unsigned k[SEL_MAX_RANKS], slot[SEL_MAX_RANKS], pre[SEL_MAX_RANKS];
#pragma unroll
    for (int r = 0; r < SEL_MAX_RANKS; ++r) {          // everything this workgroup reads of the state, before anyone rewrites it
        const bool live = r < rk.R;
        slot[r] = (PASS != 0 && live) ? st.slot_of[r] : 0u;
        k[r] = !live ? 0u : PASS == 0 ? rk.k[r] : st.rem[r];
        pre[r] = (PASS != 0 && live) ? st.slot_prefix[slot[r]] : 0u;
    }
    if (t < SEL_MAX_RANKS) { newp[t] = 0u; newrem[t] = 0u; }
    for (int s = 0; s < ns; ++s) {
        unsigned sum = 0u;
        for (int j = 0; j < 8; ++j) sum += g[s * SEL_BINS + t * 8 + j];
        part[s][t] = sum;
    }
    __syncthreads();
    if (t < ns) {                                       // exclusive scan of the 256 partial sums of slot t
        unsigned run = 0u;
        for (int i = 0; i < 256; ++i) { const unsigned v = part[t][i]; part[t][i] = run; run += v; }
    }
    __syncthreads();
    for (int r = 0; r < rk.R; ++r) {
        unsigned lo = part[slot[r]][t];
        for (int j = 0; j < 8; ++j) {
            const unsigned v = g[slot[r] * SEL_BINS + t * 8 + j];
            if (k[r] >= lo && k[r] - lo < v) { newp[r] = (pre[r] << bits) | (unsigned)(t * 8 + j); newrem[r] = k[r] - lo; }      // exactly one bin of one thread
            lo += v;
        }
    }
    __syncthreads();
    if (t != 0) return;
    if (PASS == 2) {
        const bool any_nan = st.nan != 0u;
        for (int r = 0; r < rk.R; ++r) out[(long long)c * rk.R + r] = any_nan ? NAN : sel_value(newp[r]);
        return;
    }
    unsigned n_new = 0u;
    for (int r = 0; r < rk.R; ++r) {
        unsigned s = 0u;
        while (s < n_new && st.slot_prefix[s] != newp[r]) ++s;
        if (s == n_new) st.slot_prefix[n_new++] = newp[r];
        st.slot_of[r] = s;
        st.rem[r] = newrem[r];
    }
    st.nslots = n_new;
}

// os: [C][2 P] order statistics {lower, upper} per percentile; table: [C][P].  SEL_LERP_TORCH: at::lerp as torch.quantile's CPU kernel evaluates it, one fused
// multiply-add on the fp32 weight (w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b)).  SEL_LERP_NUMPY: numpy's _lerp on an fp32 array with an fp64 weight:
// b - a rounded to fp32, then a + d t in fp64 (b - d (1 - t) where t >= 0.5), every step rounded on its own, one final rounding to fp32.
__global__ void __launch_bounds__(64) percentile_lerp_kernel(const float* __restrict__ os, int C, SelLerp p, float* __restrict__ table) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= C * p.P) return;
    const float a = os[2 * i], b = os[2 * i + 1];
    const float d = b - a;
    const double t = p.w[i % p.P];
    float r;
    if (p.mode == SEL_LERP_TORCH) {
        const float w = (float)t;
        r = w < 0.5f ? fmaf(w, d, a) : fmaf(w - 1.0f, d, b);
    } else {
        const double dd = (double)d;
        double v = dd * t;
        v = (double)a + v;
        if (t >= 0.5) {
            double u = 1.0 - t;
            u = dd * u;
            v = (double)b - u;
        }
        r = (float)v;
    }
    table[i] = r;
}

}  // namespace mh
