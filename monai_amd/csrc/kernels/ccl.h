// Connected components of a batch of 3-D (or 2-D) masks: the labelling primitive behind KeepLargestConnectedComponent (monai/transforms/post/array.py:239-354,
// get_largest_connected_component_mask, monai/transforms/utils.py:1134-1180: skimage.measure.label on the host, cuCIM + CuPy on a CUDA device), FillHoles
// (post/array.py:503-578, fill_holes, transforms/utils.py:1504-1560: scipy's iterated binary_dilation from the border, label by label, on the host) and
// LabelFilter (post/array.py:445-500).  Every kernel is batched over a leading ITEM index (blockIdx.y), as in edt.h: one item is one volume -- a channel,
// or one class selection of a label map.
//
//   cc_rows_kernel    one wave per contiguous row: the class id of every voxel from the item's rule, runs of one class from a wave scan (prefix-max of
//                     the run starts, as edt_row_kernel finds its features); link[i] = 1 + index of the run's first voxel, 0 for background
//   cc_unite_kernel   one thread per voxel: unites it with the voxels of the four earlier neighbour rows that `connectivity` admits (13 of the 26
//                     neighbours; the 13 later ones are somebody else's earlier ones), skipping every union the neighbouring voxel of the same run makes
//                     anyway.  Union-find on the link words: find with path halving, links lowered with an integer atomic min (Playne, Hawick 2018)
//   cc_flatten_kernel every voxel to its root, in place: labels[i] = 1 + the smallest linear index of the component, the same on every run
//   cc_zero_kernel / cc_count_kernel   records at root positions: int32 voxel count (integer adds of whole stretches of one label) and a
//                     touches-the-border flag
//   cc_keep_kernel    zero every selected voxel whose root is not in a short per-item list of roots
//   cc_fill_kernel    write a value into every voxel of a component that does not touch the border
//   cc_filter_kernel  the label-list selection on its own
//
// Visibility between workgroups (L1 is per CU, L2 per XCD): the link words change during cc_unite_kernel and cc_flatten_kernel, and inside these two they
// are touched ONLY by relaxed agent-scope atomic loads / stores and returned atomics (cc_ld, cc_st, cc_min); everything else is handed over across a kernel
// boundary.  No workgroup waits for another one: a union retries only after its own atomic min has lowered a link, so each trip makes progress.
// A link only ever drops to a smaller index of the same component, so the root is the component's smallest index whatever the order of the atomics.
#pragma once
#include "common.h"

namespace mh {

enum { CC_F32 = 0, CC_U8 = 1, CC_I64 = 2, CC_BOOL = 3 };
enum { CC_GT = 0, CC_EQ = 1, CC_NE = 2, CC_LIST_VALUE = 3, CC_LIST_ANY = 4, CC_VALUE = 5, CC_NUM_RULES = 6 };
enum { CC_MAX_LABELS = 32, CC_FILL_VALUE = 0, CC_FILL_BINARY = 1 };

// one row of an item table (48 x 8 bytes, built on the host)
struct CcItem {
    long long off;                  // voxel offset of the item in the label / record buffers
    long long src_off;              // element offset of the item's volume in the source tensor
    long long d, h, w;              // extent (d = 1 at rank 2)
    long long rule;                 // CC_GT .. CC_VALUE
    long long nlab;                 // entries of lab[] in use
    double v;                       // CC_EQ / CC_NE: the value compared with
    double fill;                    // cc_fill_kernel: the value written (CC_FILL_VALUE)
    long long fill_mode;            // cc_fill_kernel: CC_FILL_VALUE or CC_FILL_BINARY
    long long spare[6];
    double lab[CC_MAX_LABELS];      // CC_LIST_*: the labels (distinct)
};

#ifdef MH_SIMT_EMULATOR
// workgroups run on several host threads there: real atomics on the compiler's builtins
__device__ __forceinline__ int cc_ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void cc_st(int* p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
__device__ __forceinline__ int cc_min(int* p, int v) {
    int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
__device__ __forceinline__ void cc_add(int* p, int v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
__device__ __forceinline__ void cc_flag(unsigned char* p) { __atomic_store_n(p, (unsigned char)1, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ int cc_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_st(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cc_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_add(int* p, int v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_flag(unsigned char* p) { *p = 1; }        // every writer stores the same byte
#endif

// class id of a value under the item's rule: 0 background; CC_LIST_VALUE: 1 + the position of the value in the list (one id per listed value);
// CC_VALUE: 1 for every non-zero value -- there the value itself is the class, and cc_by_value() makes the kernels compare the raw values as well
template <typename T>
__device__ __forceinline__ int cc_class(const CcItem& it, T raw) {
    const double x = (double)raw;
    switch ((int)it.rule) {
    case CC_GT: return x > 0.0 ? 1 : 0;
    case CC_EQ: return x == it.v ? 1 : 0;
    case CC_NE: return x != it.v ? 1 : 0;
    case CC_VALUE: return x != 0.0 ? 1 : 0;
    default: {
        const int n = (int)it.nlab;
        for (int k = 0; k < n; ++k)
            if (x == it.lab[k]) return it.rule == CC_LIST_VALUE ? k + 1 : 1;
        return 0;
    }
    }
}

// several classes inside one item: two foreground voxels are of one class only if their raw values are equal too
__device__ __forceinline__ bool cc_by_value(const CcItem& it) { return it.rule == CC_LIST_VALUE || it.rule == CC_VALUE; }

// ---------------------------------------------------------------------------------------------------------------- runs
// grid (blocks of 4 rows, items), 256 threads = 4 waves = 4 rows at a time; item: off, src_off, d h w, rule.  link int32, item-relative indices + 1
template <typename T>
__global__ void __launch_bounds__(256) cc_rows_kernel(const T* __restrict__ src, const CcItem* __restrict__ items, int* __restrict__ link) {
    const CcItem& it = items[blockIdx.y];
    const int w = (int)it.w, lane = threadIdx.x & 63, chunks = (w + 63) / 64;
    const long long rows = it.d * it.h;
    for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long long)gridDim.x * 4) {      // a whole wave per row: no workgroup barrier
        const long long base = row * w;
        int carry = -1, last = 0;                              // start of the run that reaches into this chunk; class of the voxel before the chunk
        double lastv = 0.0;                                    // ... and its value (CC_VALUE: a change of value starts a run as a change of class does)
        const bool by_value = it.rule == CC_VALUE;
        for (int ch = 0; ch < chunks; ++ch) {
            const int x = ch * 64 + lane;
            const double val = x < w ? (double)src[it.src_off + base + x] : 0.0;
            const int cls = x < w ? cc_class<double>(it, val) : 0;
            int prev = __shfl(cls, lane > 0 ? lane - 1 : 0);
            double pval = __shfl(val, lane > 0 ? lane - 1 : 0);
            if (lane == 0) { prev = last; pval = lastv; }
            int v = (cls != 0 && (cls != prev || (by_value && val != pval))) ? x : -1;      // a run starts here
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl(v, lane >= o ? lane - o : lane);
                if (lane >= o) v = max(v, t);
            }
            v = max(v, carry);                                 // a foreground voxel always finds the start of its own run: a class change starts a new one
            carry = __shfl(v, 63);
            last = __shfl(cls, 63);
            lastv = __shfl(val, 63);
            if (x < w) link[it.off + base + x] = cls ? (int)(base + v) + 1 : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- union-find
// link words hold 1 + parent index; a root points at itself
__device__ __forceinline__ int cc_find(int* link, int x) {
    int p = cc_ld(link + x) - 1;
    while (p != x) {
        const int g = cc_ld(link + p) - 1;
        if (g == p) return p;
        cc_min(link + x, g + 1);                              // path halving: x skips its parent (a smaller index of the same component)
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void cc_unite(int* link, int a, int b) {
    for (;;) {
        a = cc_find(link, a);
        b = cc_find(link, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = cc_min(link + a, b + 1) - 1;          // hang the larger root under the smaller
        if (old == a) return;                                 // a was still a root
        a = old;                                              // somebody lowered a first: its former parent still has to meet b
    }
}

// grid (blocks, items), grid-stride over the voxels; item: off, src_off, d h w, rule.  MULTI: some item of the launch holds several classes
// (cc_by_value: CC_LIST_VALUE, CC_VALUE) and there the raw values tell them apart -- decided per item, so a table may mix rules; otherwise every
// foreground voxel of an item is of one class and link != 0 alone says foreground
template <typename T, bool MULTI>
__global__ void __launch_bounds__(256) cc_unite_kernel(const T* __restrict__ src, const CcItem* __restrict__ items, int connectivity, int* __restrict__ link_all) {
    const CcItem& it = items[blockIdx.y];
    const int d = (int)it.d, h = (int)it.h, w = (int)it.w;
    const long long nvox = (long long)d * h * w, hw = (long long)h * w;
    int* link = link_all + it.off;
    const T* s = src + it.src_off;
    const bool by_value = MULTI && cc_by_value(it);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        if (cc_ld(link + i) == 0) continue;
        const int z = (int)(i / hw), r = (int)(i - (long long)z * hw), y = r / w, x = r - y * w;
        const T mine = s[i];
        // same(j): voxel j is foreground of my class
#define CC_SAME(j) (cc_ld(link + (j)) != 0 && (!by_value || s[(j)] == mine))
        const bool left = x > 0 && CC_SAME(i - 1), right = x + 1 < w && CC_SAME(i + 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dz = k < 3 ? -1 : 0, dy = k < 3 ? k - 1 : -1;
            const int hops = (dz != 0) + (dy != 0);
            if (hops > connectivity || z + dz < 0 || y + dy < 0 || y + dy >= h) continue;
            const long long j = i + dz * hw + (long long)dy * w;
            if (CC_SAME(j)) {
                // the voxel to my left makes this union when it is of my run and sits under a voxel of j's run
                if (!(left && CC_SAME(j - 1))) cc_unite(link, (int)i, (int)j);
            } else if (hops + 1 <= connectivity) {
                // diagonals along the row count only where the voxel straight across is not mine; my run neighbour has them straight across
                if (x > 0 && !left && CC_SAME(j - 1)) cc_unite(link, (int)i, (int)(j - 1));
                if (x + 1 < w && !right && CC_SAME(j + 1)) cc_unite(link, (int)i, (int)(j + 1));
            }
        }
#undef CC_SAME
    }
}

// in place: a voxel's word becomes 1 + its root, which is still a valid link for everybody who walks through it meanwhile
__global__ void __launch_bounds__(256) cc_flatten_kernel(const CcItem* __restrict__ items, int* __restrict__ link_all) {
    const CcItem& it = items[blockIdx.y];
    const long long nvox = it.d * it.h * it.w;
    int* link = link_all + it.off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        int p = cc_ld(link + i) - 1;
        if (p < 0 || p == (int)i) continue;
        for (;;) {
            const int g = cc_ld(link + p) - 1;
            if (g == p) break;
            p = g;
        }
        cc_st(link + i, p + 1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- records
__global__ void __launch_bounds__(256) cc_zero_kernel(const CcItem* __restrict__ items, int* __restrict__ sizes, unsigned char* __restrict__ border) {
    const CcItem& it = items[blockIdx.y];
    const long long nvox = it.d * it.h * it.w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        sizes[it.off + i] = 0;
        border[it.off + i] = 0;
    }
}

// grid (blocks, items); every wave walks CC_COUNT_TRIPS consecutive 64-voxel trips and adds the length of each stretch of one label it sees with ONE
// integer add -- a stretch that runs on into the next trip is carried along, so a component that spans the volume costs one add per 2048 voxels and not
// one per voxel (a sum of integers: the same whatever the order).  rank: the border is that of the item's own rank (the leading extent of a rank-2
// item is no border)
enum { CC_COUNT_TRIPS = 32 };
__global__ void __launch_bounds__(256) cc_count_kernel(const int* __restrict__ labels, const CcItem* __restrict__ items, int rank, int* __restrict__ sizes,
                                                        unsigned char* __restrict__ border) {
    const CcItem& it = items[blockIdx.y];
    const int d = (int)it.d, h = (int)it.h, w = (int)it.w, lane = threadIdx.x & 63;
    const long long nvox = (long long)d * h * w, hw = (long long)h * w;
    const long long chunks = (nvox + 64 * CC_COUNT_TRIPS - 1) / (64 * CC_COUNT_TRIPS);
    for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < chunks; c += (long long)gridDim.x * 4) {      // a whole wave per chunk: no workgroup barrier
        int carry_lab = 0, carry_cnt = 0;                     // the stretch that reaches the end of the previous trip (wave-uniform)
        for (int t = 0; t < CC_COUNT_TRIPS; ++t) {
            const long long i = (c * CC_COUNT_TRIPS + t) * 64 + lane;
            if (i - lane >= nvox) break;                      // wave-uniform
            const int lab = i < nvox ? labels[it.off + i] : 0;
            const int prev = __shfl(lab, lane > 0 ? lane - 1 : 0);
            const bool head = lane == 0 || lab != prev;
            int nxt = __shfl(head ? lane : 64, lane + 1 < 64 ? lane + 1 : lane);      // the next head after this lane
            if (lane == 63) nxt = 64;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl(nxt, lane + o < 64 ? lane + o : lane);
                if (lane + o < 64) nxt = min(nxt, u);
            }
            int cnt = nxt - lane;                             // of the stretch this lane heads
            if (lane == 0) {
                if (lab == carry_lab) cnt += carry_cnt;       // the carried stretch goes on
                else if (carry_lab > 0) cc_add(sizes + it.off + carry_lab - 1, carry_cnt);
            }
            const bool last = head && nxt == 64;              // exactly one lane: its stretch is carried on
            if (head && !last && lab > 0) cc_add(sizes + it.off + lab - 1, cnt);
            int keep = last ? cnt : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) keep = max(keep, __shfl_xor(keep, o));
            carry_cnt = keep;
            carry_lab = __shfl(lab, 63);
            if (lab > 0) {
                const int z = (int)(i / hw), r = (int)(i - (long long)z * hw), y = r / w, x = r - y * w;
                const bool edge = x == 0 || x == w - 1 || (rank >= 2 && (y == 0 || y == h - 1)) || (rank >= 3 && (z == 0 || z == d - 1));
                if (edge) cc_flag(border + it.off + lab - 1);
            }
        }
        if (lane == 0 && carry_lab > 0) cc_add(sizes + it.off + carry_lab - 1, carry_cnt);
    }
}

// ---------------------------------------------------------------------------------------------------------------- apply
// keep int32 [items][nkeep]: root labels (1 + index) to keep, anything <= 0 is padding.  A labelled voxel whose root is not listed becomes 0 in `data`
template <typename T>
__global__ void __launch_bounds__(256) cc_keep_kernel(T* __restrict__ data, const int* __restrict__ labels, const int* __restrict__ keep, int nkeep,
                                                       const CcItem* __restrict__ items) {
    const CcItem& it = items[blockIdx.y];
    const long long nvox = it.d * it.h * it.w;
    const int* mine = keep + (long long)blockIdx.y * nkeep;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        const int lab = labels[it.off + i];
        if (lab <= 0) continue;
        bool kept = false;
        for (int k = 0; k < nkeep; ++k) kept = kept || mine[k] == lab;
        if (!kept) data[it.src_off + i] = (T)0;
    }
}

// CC_FILL_VALUE: `fill` into every voxel of a component that does not touch the border.  CC_FILL_BINARY: the whole volume becomes 1 outside the
// labelled mask and inside such components, 0 elsewhere (a one-hot channel after FillHoles)
template <typename T>
__global__ void __launch_bounds__(256) cc_fill_kernel(T* __restrict__ data, const int* __restrict__ labels, const unsigned char* __restrict__ border,
                                                       const CcItem* __restrict__ items) {
    const CcItem& it = items[blockIdx.y];
    const long long nvox = it.d * it.h * it.w;
    const T value = (T)it.fill;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvox; i += (long long)gridDim.x * 256) {
        const int lab = labels[it.off + i];
        const bool enclosed = lab > 0 && border[it.off + lab - 1] == 0;
        if (it.fill_mode == CC_FILL_BINARY) data[it.src_off + i] = (lab == 0 || enclosed) ? (T)1 : (T)0;
        else if (enclosed) data[it.src_off + i] = value;
    }
}

struct CcLabels {
    int n;
    double lab[CC_MAX_LABELS];
};

// out = value if it is in the list, else 0
template <typename T>
__global__ void __launch_bounds__(256) cc_filter_kernel(const T* __restrict__ src, T* __restrict__ dst, long long n, CcLabels ls) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const T raw = src[i];
        const double x = (double)raw;
        bool in = false;
        for (int k = 0; k < ls.n; ++k) in = in || x == ls.lab[k];
        dst[i] = in ? raw : (T)0;
    }
}

}  // namespace mh
