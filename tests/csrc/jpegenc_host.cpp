// maggie_amd/csrc/jpegenc.hip compiled for the host: the kernel source itself, one thread per lane of the workgroup, a barrier for __syncthreads,
// the wave's ballot and shuffle through a shared array between two barriers of the wave's 64 threads, the atomics as host atomics, the workgroups
// of a launch one after the other. Built with -fsanitize=address,undefined -pthread by tests/test_jpegenc_cpu.py and run on buffers of exactly the
// sizes the entry points are told, so that an access outside them stops the program. Not a GPU program: nothing here is launched.
//
//   jpegenc_host IN OUT   IN: int32 ncases, then per case int32 {h, w, frames, noise channels (0 = no noise), has_lut}, int32 qtab[128], the frames
//                         (uint8 [frames][h][w][3]), the lut (uint8 [3][256]) and the noise (int16 [h][w][channels]) where present.
//                         OUT: per case int32 {rc_coef, rc_bits, rc_pack, rc_stuff}, int64 {blocks per frame, raw_stride, out bytes}, int64 sizes[4][frames],
//                         int16 coef[frames][blocks][64], int32 bits[frames][blocks], int64 offs[frames][blocks], uint8 raw[frames][raw_stride],
//                         uint8 out[out bytes] (the host sequence of maggie_amd/utils/jpegenc.py).
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
#define MG_CHECK_LAUNCH() do { } while (0)
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
struct uint4 { uint32_t x, y, z, w; };
typedef void* hipStream_t;
static thread_local dim3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

constexpr int LANES = 1024;                                         // the largest workgroup (the scans); a launch uses the first `threads` of them
static pthread_barrier_t g_start, g_done, g_block, g_wave[LANES / 64];
static std::function<void()> g_body;
static int g_blocks, g_threads;
static bool g_quit = false;
static long long g_x[LANES];

static inline void __syncthreads() { pthread_barrier_wait(&g_block); }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline unsigned __umulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
static inline int __clz(int v) { return v ? __builtin_clz((unsigned)v) : 32; }
static inline int __clzll(unsigned long long v) { return v ? __builtin_clzll(v) : 64; }
// every lane of the wave calls these together
static inline unsigned long long __ballot(int pred) {
    const int l = (int)threadIdx.x, w = l >> 6;
    g_x[l] = pred ? 1 : 0;
    pthread_barrier_wait(&g_wave[w]);
    unsigned long long m = 0;
    for (int i = 0; i < 64; ++i) m |= (unsigned long long)g_x[64 * w + i] << i;
    pthread_barrier_wait(&g_wave[w]);
    return m;
}
template <typename T> static inline T __shfl_up(T v, int delta, int) {
    const int l = (int)threadIdx.x, w = l >> 6;
    g_x[l] = (long long)v;
    pthread_barrier_wait(&g_wave[w]);
    const T r = (l & 63) >= delta ? (T)g_x[l - delta] : v;
    pthread_barrier_wait(&g_wave[w]);
    return r;
}

static void worker(int tid) {
    for (;;) {
        pthread_barrier_wait(&g_start);
        if (g_quit) return;
        if (tid < g_threads)
            for (int b = 0; b < g_blocks; ++b) {
                threadIdx.x = (unsigned)tid; blockIdx.x = (unsigned)b;
                g_body();
                pthread_barrier_wait(&g_block);                         // the next workgroup reuses the `__shared__` storage
            }
        pthread_barrier_wait(&g_done);
    }
}
static void emu_launch(unsigned blocks, unsigned threads, std::function<void()> body) {
    if (threads > (unsigned)LANES || threads % 64) { fprintf(stderr, "emu: workgroup of %u lanes\n", threads); exit(3); }
    g_body = body; g_blocks = (int)blocks; g_threads = (int)threads;
    blockDim = dim3(threads); gridDim = dim3(blocks);
    pthread_barrier_destroy(&g_block);
    pthread_barrier_init(&g_block, nullptr, threads);
    pthread_barrier_wait(&g_start);
    pthread_barrier_wait(&g_done);
}
#define hipLaunchKernelGGL(k, g, b, sh, st, ...) emu_launch((g).x, (b).x, [=]() { k(__VA_ARGS__); })

#include "../../maggie_amd/csrc/jpegenc.hip"

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
    if (argc != 3) { fprintf(stderr, "usage: jpegenc_host IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    pthread_barrier_init(&g_start, nullptr, LANES + 1);
    pthread_barrier_init(&g_done, nullptr, LANES + 1);
    pthread_barrier_init(&g_block, nullptr, LANES);
    for (auto& b : g_wave) pthread_barrier_init(&b, nullptr, 64);
    std::vector<std::thread> pool;
    for (int t = 0; t < LANES; ++t) pool.emplace_back(worker, t);
    int32_t ncases = 0;
    if (!rd(in, &ncases, 4)) return 2;
    int rc_main = 0;
    for (int c = 0; c < ncases && rc_main == 0; ++c) {
        int32_t hd[5];
        if (!rd(in, hd, sizeof hd)) { rc_main = 2; break; }
        const int h = hd[0], w = hd[1], nc = hd[3], has_lut = hd[4];
        const long T = hd[2];
        const long nblk = (long)((w + 15) / 16) * ((h + 15) / 16) * 6;
        const long stride = ((nblk * MG_JPEGENC_MAX_BLOCK_BITS + 7) / 8 + 4 + 15) / 16 * 16;
        const long chunks = (stride + MG_JPEGENC_CHUNK_BYTES - 1) / MG_JPEGENC_CHUNK_BYTES;
        Exact<int32_t> qtab(128);
        Exact<uint8_t> frames((size_t)(T * h * w * 3)), lut(has_lut ? 768 : 0);
        Exact<int16_t> noise((size_t)(nc ? (long)h * w * nc : 0));
        if (!rd(in, qtab.p, 512) || !rd(in, frames.p, frames.n) || !rd(in, lut.p, lut.n) || !rd(in, noise.p, noise.n * 2)) { rc_main = 2; break; }
        Exact<int16_t> coef((size_t)(T * nblk * 64));
        Exact<int32_t> bits((size_t)(T * nblk)), ff((size_t)(T * chunks));
        Exact<int64_t> offs((size_t)(T * nblk)), sizes((size_t)(4 * T)), ch((size_t)(T * chunks));
        Exact<uint8_t> raw((size_t)(T * stride), true);
        const int rc1 = mg_jpegenc_coef(frames.p, has_lut ? lut.p : nullptr, nc ? noise.p : nullptr, nc ? nc : 1, qtab.p, coef.p, (long)coef.n, T, h, w, nullptr);
        const int rc2 = rc1 ? 0 : mg_jpegenc_bits(coef.p, (long)coef.n, bits.p, offs.p, sizes.p, T, h, w, nullptr);
        const int rc3 = rc1 || rc2 ? 0 : mg_jpegenc_pack(coef.p, (long)coef.n, bits.p, offs.p, sizes.p, raw.p, stride, ff.p, ch.p, T, h, w, nullptr);
        long total = 0, longest = 1;
        if (!rc1 && !rc2 && !rc3)
            for (long t = 0; t < T; ++t) { total += sizes.p[t]; longest = sizes.p[T + t] > longest ? sizes.p[T + t] : longest; }
        Exact<uint8_t> blob((size_t)total, true);
        long gc = (longest + MG_JPEGENC_CHUNK_BYTES - 1) / MG_JPEGENC_CHUNK_BYTES;
        gc = gc > chunks ? chunks : gc;
        const int rc4 = rc1 || rc2 || rc3 ? 0 : mg_jpegenc_stuff(raw.p, stride, ch.p, sizes.p, blob.p, total, T, h, w, gc, nullptr);
        const int32_t res[4] = {rc1, rc2, rc3, rc4};
        const int64_t dims[3] = {nblk, stride, total};
        fwrite(res, 4, 4, out);
        fwrite(dims, 8, 3, out);
        fwrite(sizes.p, 8, sizes.n, out);
        fwrite(coef.p, 2, coef.n, out);
        fwrite(bits.p, 4, bits.n, out);
        fwrite(offs.p, 8, offs.n, out);
        fwrite(raw.p, 1, raw.n, out);
        fwrite(blob.p, 1, (size_t)total, out);
    }
    g_quit = true;
    pthread_barrier_wait(&g_start);
    for (auto& t : pool) t.join();
    fclose(in);
    fclose(out);
    if (rc_main == 0) printf("jpegenc_host: ok\n");
    return rc_main;
}
