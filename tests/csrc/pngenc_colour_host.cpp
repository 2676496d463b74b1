// The colour entries of maggie_amd/csrc/pngenc.hip (mg_pngenc_size_rgb, mg_pngenc_emit_rgb) compiled for the host, with this file's own copy of
// the shim of pngenc_host.cpp: the kernel source itself, one thread per lane of the workgroup, a barrier for __syncthreads, the cross-lane scans
// through a shared array, the atomics as host atomics, the workgroups of a launch one after the other. Built with
// -fsanitize=address,undefined -pthread by tests/test_cutout_cpu.py and run on buffers of exactly the sizes the entry points are told, so that
// an access outside them stops the program. Not a GPU program: nothing here is launched.
//
//   pngenc_colour_host IN OUT    IN: int32 ncases, then per case int32 {h, w, images, channels} and the images (uint8 [images][h][w][channels]).
//                                OUT: per case int32 {rc_size, rc_emit, blocks per image, blob bytes}, int64 sizes[images],
//                                int32 recs[images][blocks][88], uint8 blob[blob bytes] (the host sequence of maggie_amd/utils/pngenc.py).
#define MG_HOST_EMU 1
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>
#include <thread>
#include <vector>

#include "../../include/maggie_hip.h"

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
#define MG_DEVCONST static const
#define MG_CHECK_LAUNCH() do { } while (0)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int LANES = MG_PNGENC_THREADS;
static pthread_barrier_t g_start, g_done, g_block;
static std::function<void()> g_body;
static int g_blocks;
static bool g_quit = false;
static int g_x[LANES];

static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicAdd(unsigned long long* p, unsigned long long v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }

namespace {
// the three scans of pngenc.hip: every lane of the workgroup calls them together
inline int pe_scan_add_excl(int v, int* total, int*) {
    const int l = (int)threadIdx.x;
    g_x[l] = v;
    __syncthreads();
    int r = 0, t = 0;
    for (int i = 0; i < LANES; ++i) { if (i < l) r += g_x[i]; t += g_x[i]; }
    __syncthreads();
    *total = t;
    return r;
}
inline int pe_scan_max_excl(int v, int*) {
    const int l = (int)threadIdx.x;
    g_x[l] = v;
    __syncthreads();
    int r = -1;
    for (int i = 0; i < l; ++i) r = g_x[i] > r ? g_x[i] : r;
    __syncthreads();
    return r;
}
inline int pe_scan_min_excl_rev(int v, int none, int*) {
    const int l = (int)threadIdx.x;
    g_x[l] = v;
    __syncthreads();
    int r = none;
    for (int i = l + 1; i < LANES; ++i) r = g_x[i] < r ? g_x[i] : r;
    __syncthreads();
    return r;
}
}  // namespace

static void worker(int tid) {
    for (;;) {
        pthread_barrier_wait(&g_start);
        if (g_quit) return;
        for (int b = 0; b < g_blocks; ++b) {
            threadIdx.x = (unsigned)tid; blockIdx.x = (unsigned)b;
            g_body();
            pthread_barrier_wait(&g_block);                             // the next workgroup reuses the `__shared__` storage
        }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(unsigned blocks, unsigned threads, std::function<void()> body) {
    if (threads != (unsigned)LANES) { fprintf(stderr, "emu: workgroup of %u lanes\n", threads); exit(3); }
    g_body = body; g_blocks = (int)blocks;
    blockDim = dim3(threads); gridDim = dim3(blocks);
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g).x, (b).x, [=]() { k(__VA_ARGS__); })

#include "../../maggie_amd/csrc/pngenc.hip"

template <typename T> struct Exact {                                // an allocation of exactly n elements, 16-byte aligned, filled with 0xA5 (or zero)
    T* p; size_t n;
    explicit Exact(size_t n_, bool zero = false) : p(nullptr), n(n_) {
        const size_t bytes = n_ ? n_ * sizeof(T) : 1;
        if (posix_memalign((void**)&p, 16, bytes)) exit(3);
        memset(p, zero ? 0 : 0xA5, bytes);
    }
    ~Exact() { free(p); }
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: pngenc_colour_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, LANES + 1);
    pthread_barrier_init(&g_done, nullptr, LANES + 1);
    pthread_barrier_init(&g_block, nullptr, LANES);
    std::vector<std::thread> pool;
    for (int t = 0; t < LANES; ++t) pool.emplace_back(worker, t);
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[4];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1], ch = hd[3];
        const long P = hd[2];
        const long nb = ((long)h * ((long)ch * w + 1) + MG_PNGENC_BLOCK_BYTES - 1) / MG_PNGENC_BLOCK_BYTES;
        Exact<uint8_t> planes((size_t)(P * h * w) * (size_t)ch);
        if (!rd(in, planes.p, planes.n)) { rc_main = 2; break; }
        Exact<int32_t> recs((size_t)(P * nb) * MG_PNGENC_REC_WORDS);
        Exact<int64_t> sizes((size_t)P);
        const int rc1 = mg_pngenc_size_rgb(planes.p, ch, P, h, w, recs.p, sizes.p, nullptr);
        long total = 0;
        if (rc1 == 0)
            for (long p = 0; p < P; ++p) total += sizes.p[p];
        const long padded = (total + 3) / 4 * 4;
        Exact<uint8_t> blob((size_t)(padded < 8 ? 8 : padded), true);
        const int rc2 = rc1 ? 0 : mg_pngenc_emit_rgb(planes.p, ch, P, h, w, recs.p, sizes.p, blob.p, (long)blob.n, nullptr);
        const int32_t res[4] = {rc1, rc2, (int32_t)nb, (int32_t)total};
        fwrite(res, 4, 4, out);
        fwrite(sizes.p, 8, sizes.n, out);
        fwrite(recs.p, 4, recs.n, out);
        fwrite(blob.p, 1, (size_t)total, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("pngenc_colour_host: ok\n");
    return rc_main;
}
