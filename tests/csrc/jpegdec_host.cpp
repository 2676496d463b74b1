// maggie_amd/csrc/jpegdec.hip compiled for the host: the kernel source itself, one thread per GPU thread, a barrier for __syncthreads, the
// workgroups of a launch one after the other. Built with -fsanitize=address,undefined -pthread by tests/test_jpegdec_cpu.py and run on buffers
// of exactly the sizes the entry points are told, so that an access outside them stops the program. Not a GPU program: nothing here is launched.
//
//   jpegdec_host IN OUT    IN: int32 ncases, then per case int32 {h, w, layout, sub_bytes, frames, blob_bytes}, int32 recs[frames][1120], blob.
//                          OUT: per case int32 {rc, status, rounds, launches, n_coef, n_planes, n_rgb}, int16 coef, uint8 planes, uint8 rgb
//                          (the host loop of maggie_amd/utils/jpegdec.py `run`; rgb only for 4:4:4 and greyscale, 4:2:0 ends in photometric.hip).
#define MG_HOST_EMU 1
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
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
struct uint2 { uint32_t x, y; };
static inline uint2 make_uint2(uint32_t a, uint32_t b) { uint2 v; v.x = a; v.y = b; return v; }
typedef void* hipStream_t;
using std::max;
using std::min;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int POOL = 256;
static pthread_barrier_t g_start, g_done, g_block[2];              // [0]: 128 lanes, [1]: 256
static std::function<void()> g_body;
static int g_threads, g_blocks;
static std::atomic<int> g_or{0};
static bool g_quit = false;

static inline pthread_barrier_t* block_barrier() { return &g_block[g_threads == POOL ? 1 : 0]; }
static inline void __syncthreads() { pthread_barrier_wait(block_barrier()); }
static inline int __syncthreads_or(int p) {
    if (p) g_or.store(1);
    __syncthreads();
    const int r = g_or.load();
    __syncthreads();
    if (threadIdx.x == 0) g_or.store(0);
    __syncthreads();
    return r;
}
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
static inline int atomicOr(int32_t* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int atomicMax(int32_t* p, int v) {
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
// pixel_norm.h's ToTensor + Normalize.norm (IEEE divisions)
static inline float mg_norm_u8(int v, float mean, float std) { return ((float)v / 255.0f - mean) / std; }

static void worker(int tid) {
    for (;;) {
        pthread_barrier_wait(&g_start);
        if (g_quit) return;
        if (tid < g_threads)
            for (int b = 0; b < g_blocks; ++b) {
                threadIdx.x = (unsigned)tid; blockIdx.x = (unsigned)b;
                g_body();
                pthread_barrier_wait(block_barrier());              // the next workgroup reuses the `__shared__` storage
            }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(unsigned blocks, unsigned threads, std::function<void()> body) {
    if (threads != 128 && threads != POOL) { fprintf(stderr, "emu: workgroup of %u lanes\n", threads); exit(3); }
    g_body = body; g_threads = (int)threads; g_blocks = (int)blocks;
    blockDim = dim3(threads); gridDim = dim3(blocks);
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g).x, (b).x, [=]() { k(__VA_ARGS__); })

#include "../../maggie_amd/csrc/jpegdec.hip"

template <typename T> struct Exact {                                // an allocation of exactly n elements (n = 0: one byte that nobody may touch)
    T* p; size_t n;
    explicit Exact(size_t n_, bool zero = false) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) { if (zero && n_) memset(p, 0, n_ * sizeof(T)); else if (n_) memset(p, 0xA5, n_ * sizeof(T)); }
    ~Exact() { free(p); }
};

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: jpegdec_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, POOL + 1);
    pthread_barrier_init(&g_done, nullptr, POOL + 1);
    pthread_barrier_init(&g_block[0], nullptr, 128);
    pthread_barrier_init(&g_block[1], nullptr, POOL);
    std::vector<std::thread> pool;
    for (int t = 0; t < POOL; ++t) pool.emplace_back(worker, t);
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[6];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1], layout = hd[2], S = hd[3];
        const long T = hd[4], nbytes = hd[5];
        Exact<int32_t> recs((size_t)T * MG_JPEGDEC_TAB_WORDS);
        Exact<uint8_t> blob((size_t)nbytes);
        if (!rd(in, recs.p, recs.n * 4) || !rd(in, blob.p, blob.n)) { rc_main = 2; break; }
        long longest = 0;
        for (long t = 0; t < T; ++t) longest = std::max<long>(longest, recs.p[t * MG_JPEGDEC_TAB_WORDS + 919]);
        const int nsub = (int)std::max<long>(1, (longest + S - 1) / S), wgs = (nsub + MG_JPEGDEC_THREADS - 1) / MG_JPEGDEC_THREADS;
        const int max_launches = wgs + 1, info_words = 4 + 2 * (max_launches + 1);
        const Geo g = geo_of(layout, h, w);
        const long nbf = (long)g.mcux * g.mcuy * g.bpm, pb = plane_bytes_of(T, layout, g);
        Exact<unsigned long long> exits((size_t)T * nsub), entries((size_t)T * wgs), bounds((size_t)2 * T * wgs, true);
        Exact<int32_t> counts((size_t)T * nsub), first((size_t)T * nsub), info((size_t)info_words, true);
        Exact<int16_t> coef((size_t)(T * nbf * 64), true);
        Exact<uint8_t> planes((size_t)pb), rgb(layout == MG_JPEGDEC_420 ? 0 : (size_t)T * h * w * 3);
        const float mean[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
        int rc = 0, k = 0;
        auto sync = [&](int launch) {
            return mg_jpegdec_sync(blob.p, nbytes, recs.p, exits.p, counts.p, entries.p, bounds.p, info.p, info_words, T, nsub, S, layout, launch, nullptr);
        };
        auto output = [&]() {
            int r = mg_jpegdec_coef(blob.p, nbytes, recs.p, exits.p, counts.p, first.p, coef.p, (long)coef.n, info.p, T, nsub, S, h, w, layout, nullptr);
            if (!r) r = mg_jpegdec_dcsum(coef.p, (long)coef.n, recs.p, T, h, w, layout, nullptr);
            if (!r) r = mg_jpegdec_idct(coef.p, (long)coef.n, recs.p, planes.p, pb, T, h, w, layout, nullptr);
            if (!r && layout != MG_JPEGDEC_420) r = mg_jpegdec_rgb(planes.p, pb, rgb.p, T, h, w, layout, MG_PHOTO_RAW, mean, std3, nullptr);
            return r;
        };
        rc = sync(0);
        if (!rc && wgs > 1) { k = 1; rc = sync(1); }
        if (!rc) rc = output();
        bool again = false;
        while (!rc && k >= 1 && info.p[2 + 2 * k] != 0) {
            if (k >= max_launches) { rc = -100; break; }                // the bound of the launches: never reached by a stream of nsub subsequences
            k += 1;
            rc = sync(k);
            again = true;
        }
        if (!rc && again) {
            memset(coef.p, 0, coef.n * 2);
            info.p[0] = 0;
            rc = output();
        }
        int rounds = 0;
        for (int q = 3; q < info_words; q += 2) rounds += info.p[q];
        const int32_t res[7] = {rc, info.p[0], rounds, k + 1, (int32_t)coef.n, (int32_t)planes.n, (int32_t)rgb.n};
        fwrite(res, 4, 7, out);
        fwrite(coef.p, 2, coef.n, out);
        fwrite(planes.p, 1, planes.n, out);
        fwrite(rgb.p, 1, rgb.n, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("jpegdec_host: ok\n");
    return rc_main;
}
