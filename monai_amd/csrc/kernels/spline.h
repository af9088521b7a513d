// Spline-order resampling, orders 0-5: what scipy.ndimage.map_coordinates(c, coords, order, mode, cval=0.0, prefilter=True) computes for a float
// image, in all eight boundary modes -- the reference's integer-`mode` branch (monai/transforms/spatial/array.py:2092-2100), which leaves the device.
//
//   prefilter (orders 2-5): fp32 image -> fp64 B-spline coefficients, one in-place pass per axis of length > 1.  Per pole z: the causal recursion
//     c+[i] = s[i] + z c+[i-1] and the anti-causal recursion c-[i] = z (c-[i+1] - c+[i]) on the signal extended infinitely by the mode's rule
//     (half-sample symmetric: reflect, grid-mirror, nearest; whole-sample symmetric: constant, grid-constant, mirror, wrap; periodic: grid-wrap).
//     The causal start is a Horner sum over SP_WARM = 48 samples of the extension (|z| <= 0.4306: 0.4306^48 < 2^-53), so a line shorter than
//     that simply walks through the extension several times; the anti-causal start is the closed form of the symmetric extensions, or the same
//     48-term sum over the periodic c+.  `nearest` and `grid-constant` filter the volume padded by SP_NPAD = 12 samples per side (edge values /
//     zeros): the pad is produced by the index arithmetic of the first pass, which reads the fp32 image; no padded copy exists.
//     One thread owns one whole line; lanes run across the fastest axis that is not filtered, so the y and z passes are coalesced.
//   sampler: one thread per output voxel, channels in the inner loop; coordinates from a 3 x 4 fp64 index matrix or a dense grid with per-axis scale
//     and offset; scipy's coordinate rule per mode, order + 1 taps per axis, neighbour indices extended by the mode's rule, fp64 accumulation, one
//     rounding to fp32.  Orders 0 and 1 read the fp32 image.  A non-finite coordinate writes NaN and reads nothing.
// No atomics, 64-bit offsets, no dependence on launch geometry: the same bits on every run.
#pragma once

namespace mh {

enum { SP_REFLECT = 0, SP_GRID_MIRROR = 1, SP_CONSTANT = 2, SP_GRID_CONSTANT = 3, SP_NEAREST = 4, SP_MIRROR = 5, SP_GRID_WRAP = 6, SP_WRAP = 7, SP_NUM_MODES = 8 };
enum { SPX_HALF = 0, SPX_WHOLE = 1, SPX_PERIODIC = 2 };
#define SP_WARM 48
#define SP_NPAD 12

struct SplineGeom {
    int NC;
    int n[3];        // image extents (z, y, x); an absent leading axis of a 2-D image has n = 1 and is neither padded nor filtered
    int N[3];        // coefficient extents: n + 2 * pad
    int pad[3];
    int present[3];
};

struct SplineFilterArgs {
    SplineGeom g;
    int axis, ext, zero_fill, npoles;
    double pole[2], gain;
};

struct SplineSampleArgs {
    SplineGeom g;
    int Do, Ho, Wo, order, mode;
    double m[12];          // affine form: index = m @ (oz, oy, ox, 1)
    double ga[3], gb[3];   // grid form: index[a] = ga[a] * grid[a] + gb[a]
};

// index i of the infinitely extended line -> [0, n)
__device__ __forceinline__ int sp_ext(int i, int n, int ext) {
    if (n <= 1) return 0;
    if (ext == SPX_PERIODIC) {
        const int m = i % n;
        return m < 0 ? m + n : m;
    }
    if (ext == SPX_HALF) {
        const int p = 2 * n;
        int m = i % p;
        if (m < 0) m += p;
        return m < n ? m : p - 1 - m;
    }
    const int p = 2 * n - 2;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - m;
}

// one pole over one line: `ld(i)` reads sample i of the line (i in [0, n)), `out` receives the result; ld may read `out` itself (every sample is read
// before it is overwritten, which is why `out` is not a __restrict__ pointer)
template <class Load>
__device__ __forceinline__ void sp_pole_pass(Load ld, double* out, long long stride, int n, double z, double gain, int ext) {
    double prev;
    if (ext == SPX_HALF && n <= SP_WARM) {
        // scipy's closed form over one period, c+[0] = s[0] + z / (1 - z^2n) * sum_i z^i (s[i] + z^n s[n-1-i]), as it evaluates it: the sum runs in s[0]'s own
        // place, so its last term (i = n - 1) reads the partial sum where s[0] is meant.  The difference is of order z^(2n-1): part of the specification for
        // short lines, below fp64 round-off for longer ones (which take the warm-up sum)
        double zn = 1.0;
        for (int i = 0; i < n; ++i) zn *= z;
        const double c0 = gain * ld(0);
        double a = c0 + zn * (gain * ld(n - 1)), zi = z;
        for (int i = 1; i < n; ++i) {
            const double other = i == n - 1 ? a : gain * ld(n - 1 - i);
            a += zi * (gain * ld(i) + zn * other);
            zi *= z;
        }
        prev = a * (z / (1.0 - zn * zn)) + c0;
    } else {
        double acc = 0.0;
        for (int k = SP_WARM; k >= 1; --k) acc = z * (gain * ld(sp_ext(-k, n, ext)) + acc);
        prev = gain * ld(0) + acc;
    }
    out[0] = prev;
    for (int i = 1; i < n; ++i) {
        prev = gain * ld(i) + z * prev;
        out[(long long)i * stride] = prev;
    }
    double c;
    if (ext == SPX_HALF) {
        c = z / (z - 1.0) * prev;
    } else if (ext == SPX_WHOLE) {
        c = z / (z * z - 1.0) * (prev + z * out[(long long)(n - 2) * stride]);
    } else {
        double acc = 0.0;
        for (int k = SP_WARM; k >= 0; --k) acc = z * (out[(long long)((n - 1 + k) % n) * stride] + acc);
        c = -acc;
    }
    out[(long long)(n - 1) * stride] = c;
    for (int i = n - 2; i >= 0; --i) {
        c = z * (c - out[(long long)i * stride]);
        out[(long long)i * stride] = c;
    }
}

// FROM_SRC: the first pass of a volume -- reads the fp32 image through the pad rule and writes every line of the coefficient volume
template <bool FROM_SRC>
__global__ void __launch_bounds__(256) spline_prefilter_kernel(const float* __restrict__ src, double* __restrict__ coef, SplineFilterArgs a) {
    const int ax = a.axis, u = ax == 0 ? 1 : 0, v = ax == 2 ? 1 : 2;       // the two other axes, v the faster one
    const long long lines = (long long)a.g.NC * a.g.N[u] * a.g.N[v];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= lines) return;
    const int qv = (int)(t % a.g.N[v]);
    const long long r = t / a.g.N[v];
    const int qu = (int)(r % a.g.N[u]);
    const long long c = r / a.g.N[u];
    const long long cs[3] = {(long long)a.g.N[1] * a.g.N[2], (long long)a.g.N[2], 1LL};
    const long long ss[3] = {(long long)a.g.n[1] * a.g.n[2], (long long)a.g.n[2], 1LL};
    double* out = coef + c * cs[0] * a.g.N[0] + qu * cs[u] + qv * cs[v];
    const int n = a.g.N[ax];
    const long long stride = cs[ax];
    auto from_coef = [&](int i) -> double { return out[(long long)i * stride]; };
    int first = 0;
    if (FROM_SRC) {
        int ju = qu - a.g.pad[u], jv = qv - a.g.pad[v];
        bool zero_line = false;
        if (ju < 0 || ju >= a.g.n[u]) { zero_line = a.zero_fill != 0; ju = ju < 0 ? 0 : a.g.n[u] - 1; }
        if (jv < 0 || jv >= a.g.n[v]) { zero_line = zero_line || a.zero_fill != 0; jv = jv < 0 ? 0 : a.g.n[v] - 1; }
        const float* line = src + c * ss[0] * a.g.n[0] + ju * ss[u] + jv * ss[v];
        const int pa = a.g.pad[ax], na = a.g.n[ax], zf = a.zero_fill;
        const long long sstride = ss[ax];
        auto from_src = [&](int i) -> double {
            int j = i - pa;
            if (j < 0 || j >= na) {
                if (zf) return 0.0;
                j = j < 0 ? 0 : na - 1;
            }
            return zero_line ? 0.0 : (double)line[(long long)j * sstride];
        };
        if (n <= 1 || a.npoles == 0) {          // nothing to filter along this axis: the cast alone
            for (int i = 0; i < n; ++i) out[(long long)i * stride] = from_src(i);
            return;
        }
        sp_pole_pass(from_src, out, stride, n, a.pole[0], a.gain, a.ext);
        first = 1;
    }
    if (n <= 1) return;
    for (int p = first; p < a.npoles; ++p) sp_pole_pass(from_coef, out, stride, n, a.pole[p], p == 0 ? a.gain : 1.0, a.ext);
}

// scipy's map_coordinate: a coordinate of the (padded) line of `len` samples under the boundary mode; the periodic and symmetric reductions are one
// exact fmod, so every finite coordinate comes back within [-1, len]
__device__ __forceinline__ double sp_map(double in, int len, int mode) {
    const double L = (double)len;
    if (in < 0.0) {
        switch (mode) {
            case SP_MIRROR:
                if (len <= 1) return 0.0;
                {
                    const double sz2 = 2.0 * L - 2.0;
                    in = fmod(in, sz2);
                    return in <= 1.0 - L ? in + sz2 : -in;
                }
            case SP_REFLECT:
            case SP_GRID_MIRROR:
                if (len <= 1) return 0.0;
                {
                    const double sz2 = 2.0 * L;
                    if (in < -sz2) in = fmod(in, sz2);
                    return in < -L ? in + sz2 : (in > -1e-15 ? 1e-15 : -in) - 1.0;
                }
            case SP_WRAP:
                if (len <= 1) return 0.0;
                return fmod(in, L - 1.0) + (L - 1.0);
            case SP_GRID_WRAP:
                if (len <= 1) return 0.0;
                return L - 1.0 - fmod(-1.0 - in, L);
            case SP_CONSTANT: return -1.0;
            default: return in;
        }
    } else if (in > L - 1.0) {
        switch (mode) {
            case SP_MIRROR:
                if (len <= 1) return 0.0;
                {
                    const double sz2 = 2.0 * L - 2.0;
                    in = fmod(in, sz2);
                    return in >= L ? sz2 - in : in;
                }
            case SP_REFLECT:
            case SP_GRID_MIRROR:
                if (len <= 1) return 0.0;
                {
                    const double sz2 = 2.0 * L;
                    in = fmod(in, sz2);
                    return in >= L ? sz2 - in - 1.0 : in;
                }
            case SP_WRAP:
                if (len <= 1) return 0.0;
                return fmod(in, L - 1.0);
            case SP_GRID_WRAP:
                if (len <= 1) return 0.0;
                return fmod(in, L);
            case SP_CONSTANT: return -1.0;
            default: return in;
        }
    }
    return in;
}

// taps of one axis at image coordinate x: false = the output is the constant 0 (outside, `constant`; nothing in reach, `grid-constant`)
template <int order>
__device__ __forceinline__ bool sp_axis_taps(double x, int N, int pad, int mode, int* __restrict__ idx, double* __restrict__ w) {
    double cc = x + (double)pad;
    if (mode == SP_GRID_CONSTANT) {
        if (cc < -(double)(order + 2) || cc > (double)(N + order + 2)) return false;
    } else if (mode == SP_NEAREST) {
        // the coordinate itself is left alone and every tap index is clamped: far outside all taps meet on the edge coefficient (their weights sum to 1)
        cc = cc < -(double)(order + 2) ? -(double)(order + 2) : (cc > (double)(N + order + 2) ? (double)(N + order + 2) : cc);
    } else {
        cc = sp_map(cc, N, mode);
        if (!(cc > -1.0)) return false;
        if (cc > (double)N) cc = (double)N;          // not reached: sp_map returns at most N - 1 + 1
    }
    const int start = (int)floor((order & 1) ? cc : cc + 0.5) - order / 2;
    const int ext = (mode == SP_REFLECT || mode == SP_GRID_MIRROR) ? SPX_HALF : (mode == SP_GRID_WRAP ? SPX_PERIODIC : SPX_WHOLE);
#pragma unroll
    for (int l = 0; l <= order; ++l) {
        int i = start + l;
        w[l] = order == 0 ? 1.0 : pp_weight<double>(order, cc - (double)i);
        if (i < 0 || i >= N) {
            if (mode == SP_GRID_CONSTANT) { w[l] = 0.0; i = 0; }
            else if (mode == SP_NEAREST) i = i < 0 ? 0 : N - 1;
            else i = sp_ext(i, N, ext);
        }
        idx[l] = i;
    }
    return true;
}

// four waves per SIMD (at most 128 VGPRs): without the bound the compiler hoists all (ORDER + 1)^3 coefficient loads of a channel and the cubic and quartic
// forms take 206 and 256 registers
template <int ORDER, typename TV, typename TG, bool GRID>
__global__ void __launch_bounds__(256, 4) spline_resample_kernel(const TV* __restrict__ vol, const TG* __restrict__ grid, float* __restrict__ dst, SplineSampleArgs a) {
    const long long ovol = (long long)a.Do * a.Ho * a.Wo;
    const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
    if (o >= ovol) return;
    double x[3];
    if (GRID) {
        for (int d = 0; d < 3; ++d) x[d] = a.ga[d] * (double)grid[d * ovol + o] + a.gb[d];
    } else {
        const int ox = (int)(o % a.Wo);
        const long long r = o / a.Wo;
        const int oy = (int)(r % a.Ho), oz = (int)(r / a.Ho);
        for (int d = 0; d < 3; ++d) x[d] = a.m[4 * d] * (double)oz + a.m[4 * d + 1] * (double)oy + a.m[4 * d + 2] * (double)ox + a.m[4 * d + 3];
    }
    int idx[3][ORDER + 1];
    double w[3][ORDER + 1];
    bool live = true, finite = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (!a.g.present[d]) {          // the absent leading axis of a 2-D image: one tap of weight 1
#pragma unroll
            for (int l = 0; l <= ORDER; ++l) { idx[d][l] = 0; w[d][l] = l == 0 ? 1.0 : 0.0; }
            continue;
        }
        if (!(fabs(x[d]) <= 1.7976931348623157e308)) { finite = false; live = false; }
        if (live) live = sp_axis_taps<ORDER>(x[d], a.g.N[d], a.g.pad[d], a.mode, idx[d], w[d]);
    }
    const int nz = a.g.present[0] ? ORDER + 1 : 1;
    const long long HW = (long long)a.g.N[1] * a.g.N[2], cvol = HW * a.g.N[0];
    for (int c = 0; c < a.g.NC; ++c) {
        double acc = 0.0;
        if (!finite) acc = __builtin_nan("");
        else if (live) {
            const TV* v = vol + c * cvol;
#pragma unroll
            for (int i = 0; i <= ORDER; ++i) {
                if (i < nz) {
#pragma unroll
                    for (int j = 0; j <= ORDER; ++j) {
                        const TV* row = v + idx[0][i] * HW + (long long)idx[1][j] * a.g.N[2];
                        const double wzy = w[0][i] * w[1][j];
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k <= ORDER; ++k) s += w[2][k] * (double)row[idx[2][k]];
                        acc += wzy * s;
                    }
                }
            }
        }
        dst[c * ovol + o] = (float)acc;
    }
}

}  // namespace mh
