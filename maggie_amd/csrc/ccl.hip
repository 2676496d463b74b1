// Connected-component labelling of many 2-D binary planes (maggie/utils/metric.py Conn :224-300, maggie/utils/postprocessing.py
// postprocess :66-86; skimage.measure.label semantics). Union-find whose root is the SMALLEST row-major index of its component, so the
// result does not depend on scheduling, and ranking the roots in raster order gives skimage's numbering.
//
//   tile_kernel    one workgroup per TH x TW tile: the foreground predicate is evaluated from the inputs, union-find runs in LDS (LDS
//                  atomicMin), tile-local roots are written as plane indices to par[] (-1 = background); with sizes, sz[] gets the tile-local
//                  component size at every tile-local root and 0 elsewhere
//   border_kernel  one thread per pixel on the far side of a tile border: lock-free find / atomicMin union on par[]. Every read of a parent
//                  word goes through an atomic RMW: other workgroups of this launch write those words and the XCDs' L2s are not coherent
//   flatten_kernel every pixel gets its final root in rt[] (par[] is only read here); tile-local roots that are not final add their size to
//                  the final root (integer atomics: exact, order-independent)
// then per entry point: consecutive labels (segment root counts, a per-plane scan, rank of each root inside its segment), the largest
// component per plane (one 64-bit atomicMax on (size << 32) | (0xFFFFFFFF - root): the largest wins, a tie goes to the smallest root),
// the Conn sum (fp64 per-block partials, summed per plane in a fixed order: no float atomics) or the post-process mask.
#include <limits.h>
#include "common.h"
#include "../../include/maggie_hip.h"

namespace {

constexpr int TH = 64, TW = 64, TPX = TH * TW;       // tile: 64 x 64 int32 in LDS = 16 KiB
constexpr int NT = 256;                              // threads per workgroup, every kernel
constexpr int SEG = 1024;                            // pixels per workgroup in the per-pixel kernels (4 consecutive per thread)
constexpr int LEVELS = 10;                           // Conn thresholds 0.1 .. 1.0

// np.float32(np.arange(0, 1.1, 0.1)[l]): np.arange gives l * 0.1 in float64, and numpy < 2 compares a float32 plane with that scalar in
// float32 (value-based casting). round_down takes the same values.
__device__ __forceinline__ float level_t(int l) { return (float)((double)l * 0.1); }

// ---- foreground predicates: plane q, plane-local pixel i ------------------------------------------------------------------------
struct MaskFg {
    const uint8_t* m; long HW;
    __device__ bool operator()(long q, long i) const { return m[q * HW + i] != 0; }
};
struct AlphaFg {
    const float* a; long HW; float thr;
    __device__ bool operator()(long q, long i) const { return a[q * HW + i] > thr; }
};
struct ConnFg {                                      // plane q = p * LEVELS + (level - 1): (gt >= t) & (pred >= t)
    const float* pred; const float* gt; long HW;
    __device__ bool operator()(long q, long i) const {
        const long p = q / LEVELS;
        const float t = level_t((int)(q - p * LEVELS) + 1);
        return gt[p * HW + i] >= t && pred[p * HW + i] >= t;
    }
};

__device__ __forceinline__ int lds_find(volatile int* L, int x) {
    int p = L[x];
    while (p != x) { x = p; p = L[x]; }
    return x;
}

__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + b, a);         // link the larger root under the smaller one
        if (old == b) return;
        b = old;                                     // b was linked meanwhile: join a with b's new parent
    }
}

__device__ __forceinline__ int g_read(int* p) { return __hip_atomic_fetch_min(p, INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(int* par, int x) {
    int p = g_read(par + x);
    while (p != x) { x = p; p = g_read(par + x); }
    return x;
}

__device__ __forceinline__ void g_union(int* par, int a, int b) {
    for (;;) {
        a = g_find(par, a);
        b = g_find(par, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(par + b, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;
    }
}

// grid: Q * tiles_x * tiles_y workgroups (1-D). With win: also clears the plane's winner key
template <class Fg>
__global__ __launch_bounds__(NT) void tile_kernel(Fg fg, int H, int W, int tiles_x, int tiles_per_plane, int conn8, int* __restrict__ par,
                                                  int* __restrict__ sz, unsigned long long* __restrict__ win) {
    __shared__ int L[TPX];
    const long q = blockIdx.x / tiles_per_plane;
    const int t = blockIdx.x - (int)(q * tiles_per_plane), ty0 = (t / tiles_x) * TH, tx0 = (t % tiles_x) * TW;
    if (win != nullptr && t == 0 && threadIdx.x == 0) win[q] = 0;      // the winner key (winner_kernel, a later launch)
    const int th = min(TH, H - ty0), tw = min(TW, W - tx0);
    const long HW = (long)H * W;
    constexpr int PER = TPX / NT;
    for (int k = 0; k < PER; ++k) {
        const int j = threadIdx.x + k * NT, ly = j / TW, lx = j % TW;
        L[j] = (ly < th && lx < tw && fg(q, (long)(ty0 + ly) * W + tx0 + lx)) ? j : -1;
    }
    __syncthreads();
    for (int k = 0; k < PER; ++k) {
        const int j = threadIdx.x + k * NT, ly = j / TW, lx = j % TW;
        if (L[j] < 0) continue;
        if (lx > 0 && L[j - 1] >= 0) lds_union(L, j, j - 1);
        if (ly > 0) {
            if (L[j - TW] >= 0) lds_union(L, j, j - TW);
            if (conn8) {
                if (lx > 0 && L[j - TW - 1] >= 0) lds_union(L, j, j - TW - 1);
                if (lx + 1 < tw && L[j - TW + 1] >= 0) lds_union(L, j, j - TW + 1);
            }
        }
    }
    __syncthreads();
    int root[PER];
    for (int k = 0; k < PER; ++k) {
        const int j = threadIdx.x + k * NT;
        root[k] = L[j] < 0 ? -1 : lds_find(L, j);
    }
    int* P = par + q * HW;
    for (int k = 0; k < PER; ++k) {
        const int j = threadIdx.x + k * NT, ly = j / TW, lx = j % TW;
        if (ly < th && lx < tw) {
            const int r = root[k];
            P[(long)(ty0 + ly) * W + tx0 + lx] = r < 0 ? -1 : (ty0 + r / TW) * W + tx0 + r % TW;
        }
    }
    if (sz == nullptr) return;
    __syncthreads();                                 // every find is done: L becomes the size counters
    for (int k = 0; k < PER; ++k) L[threadIdx.x + k * NT] = 0;
    __syncthreads();
    for (int k = 0; k < PER; ++k)
        if (root[k] >= 0) atomicAdd(L + root[k], 1);
    __syncthreads();
    int* S = sz + q * HW;
    for (int k = 0; k < PER; ++k) {
        const int j = threadIdx.x + k * NT, ly = j / TW, lx = j % TW;
        if (ly < th && lx < tw) S[(long)(ty0 + ly) * W + tx0 + lx] = L[j];
    }
}

// one thread per pixel (y, x) with x a tile column start (> 0) or y a tile row start (> 0); joins it with its neighbours across the border
template <class Fg>
__global__ __launch_bounds__(NT) void border_kernel(Fg fg, int H, int W, int conn8, long nv, long per_plane, long total, int* __restrict__ par) {
    const long g = (long)blockIdx.x * NT + threadIdx.x;
    if (g >= total) return;
    const long q = g / per_plane, k = g - q * per_plane;
    int y, x;
    bool vert;
    if (k < nv) { y = (int)(k % H); x = (int)(k / H + 1) * TW; vert = true; }              // column border: neighbours on the left
    else { const long m = k - nv; x = (int)(m % W); y = (int)(m / W + 1) * TH; vert = false; }  // row border: neighbours above
    const int i = y * W + x;
    if (!fg(q, i)) return;
    int* P = par + q * (long)H * W;
    if (vert) {
        if (fg(q, i - 1)) g_union(P, i, i - 1);
        if (conn8) {
            if (y > 0 && fg(q, i - W - 1)) g_union(P, i, i - W - 1);
            if (y + 1 < H && fg(q, i + W - 1)) g_union(P, i, i + W - 1);
        }
    } else {
        if (fg(q, i - W)) g_union(P, i, i - W);
        if (conn8) {
            if (x > 0 && fg(q, i - W - 1)) g_union(P, i, i - W - 1);
            if (x + 1 < W && fg(q, i - W + 1)) g_union(P, i, i - W + 1);
        }
    }
}

__device__ __forceinline__ int block_sum_int(int v, int* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += sh[w];
    __syncthreads();
    return s;
}

// grid: Q * nseg (1-D). rt[i] = final root of i (-1: background). With sz: tile-local roots that are not final add their count to the
// final root's. With segcnt: the number of final roots in each segment.
__global__ __launch_bounds__(NT) void flatten_kernel(const int* __restrict__ par, long HW, int nseg, int* __restrict__ rt, int* sz,
                                                     int* __restrict__ segcnt) {
    __shared__ int sh[NT / 64];
    const long q = blockIdx.x / nseg;
    const int s = blockIdx.x - (int)(q * nseg);
    const int* P = par + q * HW;
    int nroot = 0;
    for (int k = 0; k < SEG / NT; ++k) {
        const long i = (long)s * SEG + threadIdx.x * (SEG / NT) + k;
        if (i >= HW) break;
        int r = P[i];
        if (r >= 0) {
            int p = P[r];
            while (p != r) { r = p; p = P[r]; }
            nroot += r == i;
            if (sz != nullptr && r != i) {
                const int c = sz[q * HW + i];
                if (c > 0) atomicAdd(sz + q * HW + r, c);
            }
        }
        rt[q * HW + i] = r;
    }
    if (segcnt != nullptr) {
        const int c = block_sum_int(nroot, sh);
        if (threadIdx.x == 0) segcnt[blockIdx.x] = c;
    }
}

// grid: Q. segcnt[q][*] -> exclusive offsets in place, num[q] = total (serial over chunks of NT, block scan inside a chunk)
__global__ __launch_bounds__(NT) void seg_scan_kernel(int* __restrict__ seg, int nseg, int* __restrict__ num) {
    __shared__ int sh[NT];
    int* S = seg + (long)blockIdx.x * nseg;
    int carry = 0;
    for (int c0 = 0; c0 < nseg; c0 += NT) {
        const int j = c0 + threadIdx.x;
        const int v = j < nseg ? S[j] : 0;
        sh[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < NT; off <<= 1) {     // Hillis-Steele inclusive scan
            const int a = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += a;
            __syncthreads();
        }
        if (j < nseg) S[j] = carry + sh[threadIdx.x] - v;
        carry += sh[NT - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) num[blockIdx.x] = carry;
}

// grid: Q * nseg. Roots get their consecutive label (segment offset + raster rank inside the segment + 1). rt and labels are the same
// buffer in mg_cc_label: every thread reads its own pixels before the barrier and writes them after it.
__global__ __launch_bounds__(NT) void root_label_kernel(const int* rt, long HW, int nseg, const int* __restrict__ segoff, int* labels) {
    __shared__ int sh[NT];
    const long q = blockIdx.x / nseg;
    const int s = blockIdx.x - (int)(q * nseg);
    constexpr int PER = SEG / NT;
    const long i0 = q * HW + (long)s * SEG + threadIdx.x * PER;
    const long end = (q + 1) * HW;
    int flags = 0, n = 0;
    for (int k = 0; k < PER; ++k) {
        const long i = i0 + k;
        if (i < end && rt[i] == i - q * HW) { flags |= 1 << k; ++n; }
    }
    sh[threadIdx.x] = n;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int a = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
        __syncthreads();
        sh[threadIdx.x] += a;
        __syncthreads();
    }
    int lab = segoff[blockIdx.x] + sh[threadIdx.x] - n;
    for (int k = 0; k < PER; ++k)
        if (flags & (1 << k)) labels[i0 + k] = ++lab;
}

// labels of the non-root pixels: labels[i] still holds the root (flatten_kernel), the roots hold their label (previous launch; a final
// root is a pixel whose par[] entry is itself after the border merge). Background: 0.
__global__ __launch_bounds__(NT) void pixel_label_kernel(const int* __restrict__ par, long HW, long n, int* labels) {
    const long g = (long)blockIdx.x * NT + threadIdx.x;
    if (g >= n) return;
    const long q = g / HW;
    const int p = par[g];
    if (p < 0) labels[g] = 0;
    else if (p != g - q * HW) labels[g] = labels[q * HW + labels[g]];
}

// grid: Q * nseg. win[q] = max over final roots of (size << 32) | (0xFFFFFFFF - root)
__global__ __launch_bounds__(NT) void winner_kernel(const int* __restrict__ rt, const int* __restrict__ sz, long HW, int nseg,
                                                    unsigned long long* __restrict__ win) {
    __shared__ unsigned long long sh[NT / 64];
    const long q = blockIdx.x / nseg;
    const int s = blockIdx.x - (int)(q * nseg);
    unsigned long long best = 0;
    for (int k = 0; k < SEG / NT; ++k) {
        const long i = (long)s * SEG + k * NT + threadIdx.x;
        if (i < HW && rt[q * HW + i] == i) {
            const unsigned long long key = ((unsigned long long)(unsigned)sz[q * HW + i] << 32) | (0xFFFFFFFFull - (unsigned long long)i);
            best = key > best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) best = sh[w] > best ? sh[w] : best;
        if (best != 0) atomicMax(win + q, best);
    }
}

__device__ __forceinline__ int win_root(unsigned long long w) { return w == 0 ? -1 : (int)(0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFull)); }

// out = alpha * [pixel in the largest component]; a plane without foreground is copied unchanged
__global__ __launch_bounds__(NT) void pp_out_kernel(const float* __restrict__ alpha, const int* __restrict__ rt, long HW, long n,
                                                    const unsigned long long* __restrict__ win, float* __restrict__ out) {
    const long g = (long)blockIdx.x * NT + threadIdx.x;
    if (g >= n) return;
    const long q = g / HW;
    const unsigned long long w = win[q];
    const float a = alpha[g];
    if (w == 0) { out[g] = a; return; }
    const int r = rt[g];
    out[g] = a * ((r >= 0 && r == win_root(w)) ? 1.f : 0.f);
}

// grid: P * nseg. Per pixel: round_down = t_{i-1} for the first level i whose largest component misses it, else 1; the Conn term of
// metric.py:290-294 in fp32; fp64 partial per workgroup into slab[p * nseg + s]
__global__ __launch_bounds__(NT) void conn_term_kernel(const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ tri,
                                                       int mode, const int* __restrict__ rt, long HW, int nseg,
                                                       const unsigned long long* __restrict__ win, double* __restrict__ slab) {
    __shared__ double sh[NT / 64];
    const long p = blockIdx.x / nseg;
    const int s = blockIdx.x - (int)(p * nseg);
    int wr[LEVELS];
#pragma unroll
    for (int l = 0; l < LEVELS; ++l) wr[l] = win_root(win[p * LEVELS + l]);
    double acc = 0.0;
    for (int k = 0; k < SEG / NT; ++k) {
        const long i = (long)s * SEG + k * NT + threadIdx.x;
        if (i >= HW) break;
        float rd = 1.f;
        for (int l = 0; l < LEVELS; ++l) {
            const int r = rt[(p * LEVELS + l) * HW + i];
            if (r < 0 || r != wr[l]) { rd = level_t(l); break; }
        }
        const float g = gt[p * HW + i], q = pred[p * HW + i];
        const float gd = g - rd, pd = q - rd;
        const float gphi = 1.f - gd * (gd >= 0.15f ? 1.f : 0.f);
        const float pphi = 1.f - pd * (pd >= 0.15f ? 1.f : 0.f);
        float m = 1.f;
        if (mode != 0 && tri != nullptr) m = tri[p * HW + i] > 0.f ? 1.f : 0.f;
        acc += (double)(fabsf(gphi - pphi) * m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < NT / 64; ++w) t += sh[w];
        slab[blockIdx.x] = t;
    }
}

// grid: P. out[p] = sum of the plane's slab entries, fixed order (strided per thread, then a fixed tree)
__global__ __launch_bounds__(NT) void conn_finish_kernel(const double* __restrict__ slab, int nseg, double* __restrict__ out) {
    __shared__ double sh[NT];
    const double* S = slab + (long)blockIdx.x * nseg;
    double a = 0.0;
    for (int j = threadIdx.x; j < nseg; j += NT) a += S[j];
    sh[threadIdx.x] = a;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct Geo {
    long HW, Q;
    int tiles_x, tiles_y, nseg;
    long nv, nh;
    bool ok;
};

Geo geo(long Q, int H, int W) {
    Geo g{};
    g.ok = Q > 0 && H > 0 && W > 0 && (long)H * W < (1L << 31) - 1;
    if (!g.ok) return g;
    g.HW = (long)H * W;
    g.Q = Q;
    g.tiles_x = (W + TW - 1) / TW;
    g.tiles_y = (H + TH - 1) / TH;
    g.nseg = (int)((g.HW + SEG - 1) / SEG);
    g.nv = (long)(g.tiles_x - 1) * H;
    g.nh = (long)(g.tiles_y - 1) * W;
    return g;
}

long align256(long b) { return (b + 255) & ~255L; }

// scratch layout (bytes): label: par[Q][HW] i32 | seg[Q][nseg] i32;  largest (conn / post-process): par | rt | sz [Q][HW] i32 |
// win[Q] u64 | slab[P][nseg] f64
long scratch_bytes(int op, long P, int H, int W) {
    const long Q = op == MG_CC_OP_CONN ? P * LEVELS : P;
    const Geo g = geo(Q, H, W);
    if (!g.ok) return 0;
    const long plane = align256(Q * g.HW * 4);
    if (op == MG_CC_OP_LABEL) return plane + align256(Q * g.nseg * 4);
    return 3 * plane + align256(Q * 8) + align256(P * g.nseg * 8);
}

unsigned grid_for(long n) { return (unsigned)((n + NT - 1) / NT); }

// tile union-find + border merge + flatten: rt[q][i] = final root; sz[] (if given) final sizes at the final roots
template <class Fg>
int run_ccl(const Fg& fg, const Geo& g, int H, int W, int conn8, int* par, int* rt, int* sz, int* segcnt, unsigned long long* win,
            hipStream_t st) {
    const long tiles = (long)g.tiles_x * g.tiles_y;
    if (g.Q * tiles > 0xFFFFFFFFL || g.Q * g.nseg > 0xFFFFFFFFL) return -3;
    hipLaunchKernelGGL(tile_kernel<Fg>, dim3((unsigned)(g.Q * tiles)), dim3(NT), 0, st, fg, H, W, g.tiles_x, (int)tiles, conn8, par, sz, win);
    const long per_plane = g.nv + g.nh, total = g.Q * per_plane;
    if (total > 0) {
        if ((total + NT - 1) / NT > 0xFFFFFFFFL) return -3;
        hipLaunchKernelGGL(border_kernel<Fg>, dim3(grid_for(total)), dim3(NT), 0, st, fg, H, W, conn8, g.nv, per_plane, total, par);
    }
    hipLaunchKernelGGL(flatten_kernel, dim3((unsigned)(g.Q * g.nseg)), dim3(NT), 0, st, (const int*)par, g.HW, g.nseg, rt, sz, segcnt);
    return (int)hipGetLastError();
}

struct Largest { int *par, *rt, *sz; unsigned long long* win; double* slab; };

Largest carve(void* scratch, const Geo& g) {
    char* b = (char*)scratch;
    const long plane = align256(g.Q * g.HW * 4);
    Largest l;
    l.par = (int*)b;
    l.rt = (int*)(b + plane);
    l.sz = (int*)(b + 2 * plane);
    l.win = (unsigned long long*)(b + 3 * plane);
    l.slab = (double*)(b + 3 * plane + align256(g.Q * 8));
    return l;
}

template <class Fg>
int run_largest(const Fg& fg, const Geo& g, int H, int W, int conn8, const Largest& l, hipStream_t st) {
    const int rc = run_ccl(fg, g, H, W, conn8, l.par, l.rt, l.sz, nullptr, l.win, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(winner_kernel, dim3((unsigned)(g.Q * g.nseg)), dim3(NT), 0, st, (const int*)l.rt, (const int*)l.sz, g.HW, g.nseg, l.win);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int mg_cc_scratch_bytes(int op, int P, int H, int W, long* bytes) {
    if (op != MG_CC_OP_LABEL && op != MG_CC_OP_CONN && op != MG_CC_OP_LARGEST) return -1;
    if (P < 0 || H < 0 || W < 0) return -1;
    if ((long)H * W >= (1L << 31) - 1) return -2;
    *bytes = scratch_bytes(op, P, H, W);
    return 0;
}

extern "C" int mg_cc_label(const uint8_t* mask, int P, int H, int W, int connectivity, int32_t* labels, int32_t* num, void* scratch,
                           void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (connectivity != 1 && connectivity != 2) return -1;
    if ((long)H * W >= (1L << 31) - 1) return -2;
    if (P <= 0 || H <= 0 || W <= 0) {
        if (P > 0) return (int)hipMemsetAsync(num, 0, (size_t)P * 4, st);
        return 0;
    }
    const Geo g = geo(P, H, W);
    int* par = (int*)scratch;
    int* seg = (int*)((char*)scratch + align256(g.Q * g.HW * 4));
    MaskFg fg{mask, g.HW};
    int rc = run_ccl(fg, g, H, W, connectivity == 2, par, labels, nullptr, seg, nullptr, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(seg_scan_kernel, dim3((unsigned)g.Q), dim3(NT), 0, st, seg, g.nseg, num);
    hipLaunchKernelGGL(root_label_kernel, dim3((unsigned)(g.Q * g.nseg)), dim3(NT), 0, st, (const int*)labels, g.HW, g.nseg, (const int*)seg, labels);
    const long n = g.Q * g.HW;
    if ((n + NT - 1) / NT > 0xFFFFFFFFL) return -3;
    hipLaunchKernelGGL(pixel_label_kernel, dim3(grid_for(n)), dim3(NT), 0, st, (const int*)par, g.HW, n, labels);
    return (int)hipGetLastError();
}

extern "C" int mg_metric_conn(const float* pred, const float* gt, const float* trimap, int mask_mode, int P, int H, int W, void* scratch,
                              double* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if ((long)H * W >= (1L << 31) - 1) return -2;
    if (P <= 0) return 0;
    if (H <= 0 || W <= 0) return (int)hipMemsetAsync(out, 0, (size_t)P * 8, st);
    const Geo g = geo((long)P * LEVELS, H, W);
    const Largest l = carve(scratch, g);
    ConnFg fg{pred, gt, g.HW};
    int rc = run_largest(fg, g, H, W, 0, l, st);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(conn_term_kernel, dim3((unsigned)((long)P * g.nseg)), dim3(NT), 0, st, pred, gt, trimap, mask_mode, (const int*)l.rt, g.HW,
                       g.nseg, (const unsigned long long*)l.win, l.slab);
    hipLaunchKernelGGL(conn_finish_kernel, dim3((unsigned)P), dim3(NT), 0, st, (const double*)l.slab, g.nseg, out);
    return (int)hipGetLastError();
}

extern "C" int mg_postprocess_largest_cc(const float* alpha, int P, int H, int W, float thresh, void* scratch, float* out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if ((long)H * W >= (1L << 31) - 1) return -2;
    if (P <= 0 || H <= 0 || W <= 0) return 0;
    const Geo g = geo(P, H, W);
    const Largest l = carve(scratch, g);
    AlphaFg fg{alpha, g.HW, thresh};
    int rc = run_largest(fg, g, H, W, 1, l, st);
    if (rc != 0) return rc;
    const long n = g.Q * g.HW;
    if ((n + NT - 1) / NT > 0xFFFFFFFFL) return -3;
    hipLaunchKernelGGL(pp_out_kernel, dim3(grid_for(n)), dim3(NT), 0, st, alpha, (const int*)l.rt, g.HW, n, (const unsigned long long*)l.win, out);
    return (int)hipGetLastError();
}
