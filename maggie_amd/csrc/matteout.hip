// Matte output on the device: the pixel passes behind the reference's predictor (demo/maggie_predictor.py, demo/app.py).
//   mg_matte_composite    : `(image * a + (1 - a) * background).astype(np.uint8)` per instance (maggie_predictor.py:68-76,151-157), fused with the
//                           reverse transform and the snapping in front of it (:62-65,124-128; the arithmetic of postprocess_alpha_kernel in
//                           sparse.hip, restated here so that that kernel keeps its build and its bits).
//   mg_matte_overlay      : `Image.blend(image, palette(mask > 0), alpha)` (app.py:59-65).
//   mg_matte_label_ids    : which ids a label map holds (`np.unique`, maggie_predictor.py:35-36).
//   mg_matte_label_planes : `(bin_masks == id) * 255` per id (maggie_predictor.py:38-40).
// DESIGN.md section 29. A lane owns 16 consecutive pixels: 48 bytes of a frame (three 16-byte loads, three 16-byte stores per instance), 16 mask
// or label bytes (one load), 16 alphas (four 16-byte stores). Every wide access has a twin for a base that is not 16-byte aligned; the
// last, partial group of a frame goes pixel by pixel.
//
// The whole file is compiled WITHOUT floating-point contraction: NumPy rounds each product and the sum of the composite on its own, Pillow
// the product and the sum of the blend, and a fused multiply-add changes bytes (about one in ten thousand: DESIGN.md section 29).
// hipcc contracts by default and __fmul_rn / __fadd_rn are plain operators in HIP's headers, so the pragma is what keeps them apart.
#include "common.h"
#include "../../include/maggie_hip.h"

#pragma clang fp contract(off)

namespace {
constexpr int NT = MG_MATTE_THREADS;
constexpr int GP = MG_MATTE_GROUP;          // pixels of a lane

__device__ __forceinline__ uint4 ld16(const void* p, bool aligned) {
    if (aligned) return *(const uint4*)p;
    uint4 v;
    __builtin_memcpy(&v, p, 16);            // the address may have any alignment
    return v;
}
__device__ __forceinline__ void st16(void* p, const uint4& v, bool aligned) {
    if (aligned) *(uint4*)p = v;
    else __builtin_memcpy(p, &v, 16);
}
__device__ __forceinline__ bool is16(const void* p) { return ((uintptr_t)p & 15) == 0; }
__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xffu; }

// ---- composite -------------------------------------------------------------------------------------------------------------------------
struct Geo {
    int Hin, Win, Hc, Wc, H, W;
    float sy, sx;
    int snap, identity;
};

// F.interpolate(mode='bilinear', align_corners=True) on the cropped (Hc x Wc) plane, as postprocess_alpha_kernel states it: the four taps
// (offsets into the plane) and the two weights of the output pixel (y, x)
struct Taps { int o00, dx, dy; float ly, lx; };                // the top-left tap, the steps to its right and lower neighbours (0 at the crop's edge)
__device__ __forceinline__ Taps taps_of(const Geo& g, int y, int x) {
    Taps t;
    if (g.identity) {
        t.o00 = y * g.Win + x;
        t.dx = t.dy = 0;
        t.ly = t.lx = 0.f;
        return t;
    }
    const float fy = (float)y * g.sy, fx = (float)x * g.sx;
    int y0 = (int)fy, x0 = (int)fx;
    if (y0 > g.Hc - 1) y0 = g.Hc - 1;
    if (x0 > g.Wc - 1) x0 = g.Wc - 1;
    t.dy = y0 + 1 < g.Hc ? g.Win : 0;
    t.dx = x0 + 1 < g.Wc ? 1 : 0;
    t.ly = fy - (float)y0;
    t.lx = fx - (float)x0;
    t.o00 = y0 * g.Win + x0;
    return t;
}
__device__ __forceinline__ float alpha_of(const Geo& g, const float* __restrict__ src, const Taps& t) {
    float v;
    if (g.identity) {
        v = src[t.o00];                                         // size == crop: the value itself, bit for bit
    } else {
        const float v00 = src[t.o00], v01 = src[t.o00 + t.dx], v10 = src[t.o00 + t.dy], v11 = src[t.o00 + t.dy + t.dx];
        v = (1.f - t.ly) * ((1.f - t.lx) * v00 + t.lx * v01) + t.ly * ((1.f - t.lx) * v10 + t.lx * v11);
    }
    if (g.snap) {
        if (v <= 1.0f / 255.0f) v = 0.f;
        if (v >= 254.0f / 255.0f) v = 1.f;
    }
    return v;
}
// (image * a + (1 - a) * bg).astype(uint8): two products and a sum, each rounded to fp32; the clamp is ours (it acts only for a outside [0, 1])
__device__ __forceinline__ uint32_t blend_of(uint32_t v, uint32_t bg, float a) {
    const float t1 = (float)v * a;
    const float t2 = (1.f - a) * (float)bg;
    float s = t1 + t2;
    s = fminf(fmaxf(s, 0.f), 255.f);
    return (uint32_t)s;
}

template <bool BG_IMAGE>
__global__ __launch_bounds__(NT) void composite_kernel(const float* __restrict__ alpha, const uint8_t* __restrict__ frames,
                                                       const uint8_t* __restrict__ bg, long bg_stride, uint32_t bg_rgb, int P, Geo g,
                                                       uint8_t* __restrict__ out, float* __restrict__ aout) {
    const long t = blockIdx.y;
    const long npix = (long)g.H * g.W, n3 = npix * 3, plane = (long)g.Hin * g.Win;
    const uint8_t* fr = frames + t * n3;
    const uint8_t* bgp = BG_IMAGE ? bg + t * bg_stride : nullptr;
    const bool fr_al = is16(fr), bg_al = BG_IMAGE && is16(bgp);
    const long groups = (npix + GP - 1) / GP;
    const uint32_t c3[3] = {bg_rgb & 0xffu, (bg_rgb >> 8) & 0xffu, (bg_rgb >> 16) & 0xffu};
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long pix0 = grp * GP;
        int y = (int)(pix0 / g.W), x = (int)(pix0 - (long)y * g.W);
        if (pix0 + GP <= npix) {
            uint32_t fw[12], bw[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = ld16(fr + pix0 * 3 + 16 * q, fr_al);
                fw[4 * q] = v.x; fw[4 * q + 1] = v.y; fw[4 * q + 2] = v.z; fw[4 * q + 3] = v.w;
            }
            if (BG_IMAGE) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const uint4 v = ld16(bgp + pix0 * 3 + 16 * q, bg_al);
                    bw[4 * q] = v.x; bw[4 * q + 1] = v.y; bw[4 * q + 2] = v.z; bw[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 12; ++q)
                    bw[q] = c3[(4 * q) % 3] | c3[(4 * q + 1) % 3] << 8 | c3[(4 * q + 2) % 3] << 16 | c3[(4 * q + 3) % 3] << 24;
            }
            int o00[GP];
            float ly[GP], lx[GP];
            uint32_t right = 0, below = 0;                       // bit j: pixel j has a neighbour to the right / below inside the crop
#pragma unroll
            for (int j = 0; j < GP; ++j) {
                const Taps tj = taps_of(g, y, x);
                o00[j] = tj.o00; ly[j] = tj.ly; lx[j] = tj.lx;
                right |= (uint32_t)(tj.dx != 0) << j;
                below |= (uint32_t)(tj.dy != 0) << j;
                if (++x == g.W) { x = 0; ++y; }
            }
            for (int p = 0; p < P; ++p) {
                const long ip = t * P + p;
                const float* src = alpha + ip * plane;
                float* ad = aout ? aout + ip * npix + pix0 : nullptr;
                const bool ad_al = is16(ad);
                uint32_t ow[12];
                // what does not depend on p stays in its compact form: without these the compiler keeps every byte as a float and every tap's
                // address and (1 - l) across the instances, ~380 registers and one wave a SIMD
#pragma unroll
                for (int q = 0; q < 12; ++q) asm volatile("" : "+v"(fw[q]), "+v"(bw[q]));
#pragma unroll
                for (int j = 0; j < GP; ++j) asm volatile("" : "+v"(o00[j]), "+v"(ly[j]), "+v"(lx[j]));
                // four pixels make twelve bytes, three whole words of the output: a quad's taps, alphas and bytes die before the next quad starts
#pragma unroll
                for (int q4 = 0; q4 < GP / 4; ++q4) {
                    float a[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int jj = 4 * q4 + j;
                        const Taps tj = {o00[jj], (int)(right >> jj & 1u), (below >> jj & 1u) ? g.Win : 0, ly[jj], lx[jj]};
                        a[j] = alpha_of(g, src, tj);
                    }
                    if (ad) st16(ad + 4 * q4, make_uint4(__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])), ad_al);
#pragma unroll
                    for (int q = 3 * q4; q < 3 * q4 + 3; ++q) {
                        uint32_t w = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            const int k = 4 * q + b;
                            w |= blend_of(byte_of(fw, k), byte_of(bw, k), a[k / 3 - 4 * q4]) << (8 * b);
                        }
                        ow[q] = w;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                uint8_t* od = out + ip * n3 + pix0 * 3;
                const bool al = is16(od);
#pragma unroll
                for (int q = 0; q < 3; ++q) st16(od + 16 * q, make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]), al);
            }
        } else {
            // the last group of a frame: fewer than GP pixels, byte by byte
            const int cnt = (int)(npix - pix0);
            for (int j = 0; j < cnt; ++j) {
                const Taps tp = taps_of(g, y, x);
                const long i = pix0 + j;
                uint32_t v[3], b[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    v[c] = fr[i * 3 + c];
                    b[c] = BG_IMAGE ? (uint32_t)bgp[i * 3 + c] : c3[c];
                }
                for (int p = 0; p < P; ++p) {
                    const long ip = t * P + p;
                    const float a = alpha_of(g, alpha + ip * plane, tp);
                    if (aout) aout[ip * npix + i] = a;
#pragma unroll
                    for (int c = 0; c < 3; ++c) out[ip * n3 + i * 3 + c] = (uint8_t)blend_of(v[c], b[c], a);
                }
                if (++x == g.W) { x = 0; ++y; }
            }
        }
    }
}

// ---- overlay ---------------------------------------------------------------------------------------------------------------------------
// Image.blend: (UINT8)((float)in1 + alpha * (float)(in2 - in1)) with in2 = the colour where mask > 0, else 0
__device__ __forceinline__ uint32_t overlay_of(uint32_t in1, uint32_t colour, bool on, float alpha) {
    const int in2 = on ? (int)colour : 0;
    const float s = (float)in1 + alpha * (float)(in2 - (int)in1);
    return (uint32_t)fminf(fmaxf(s, 0.f), 255.f);
}

__global__ __launch_bounds__(NT) void overlay_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ masks, long npix,
                                                     uint32_t rgb, float alpha, uint8_t* __restrict__ out) {
    const bool fr_al = is16(frames), m_al = is16(masks), o_al = is16(out);
    const long groups = (npix + GP - 1) / GP;
    const uint32_t c3[3] = {rgb & 0xffu, (rgb >> 8) & 0xffu, (rgb >> 16) & 0xffu};
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long pix0 = grp * GP;
        if (pix0 + GP <= npix) {
            uint32_t fw[12], mw[4], ow[12];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = ld16(frames + pix0 * 3 + 16 * q, fr_al);
                fw[4 * q] = v.x; fw[4 * q + 1] = v.y; fw[4 * q + 2] = v.z; fw[4 * q + 3] = v.w;
            }
            const uint4 m = ld16(masks + pix0, m_al);
            mw[0] = m.x; mw[1] = m.y; mw[2] = m.z; mw[3] = m.w;
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int k = 4 * q + b;
                    w |= overlay_of(byte_of(fw, k), c3[k % 3], byte_of(mw, k / 3) != 0, alpha) << (8 * b);
                }
                ow[q] = w;
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) st16(out + pix0 * 3 + 16 * q, make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]), o_al);
        } else {
            for (long i = pix0; i < npix; ++i) {
                const bool on = masks[i] != 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) out[i * 3 + c] = (uint8_t)overlay_of(frames[i * 3 + c], c3[c], on, alpha);
            }
        }
    }
}

// ---- label maps ------------------------------------------------------------------------------------------------------------------------
// Sixteen labels of a lane, from a uint8 or an int32 map; a label outside 0..255 comes back as -1.
template <typename T> struct Labels;
template <> struct Labels<uint8_t> {
    static __device__ __forceinline__ void load(const uint8_t* p, bool al, int* id) {
        const uint4 v = ld16(p, al);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < GP; ++j) id[j] = (int)byte_of(w, j);
    }
    static __device__ __forceinline__ int one(const uint8_t* p) { return *p; }
};
template <> struct Labels<int32_t> {
    static __device__ __forceinline__ void load(const int32_t* p, bool al, int* id) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = ld16(p + 4 * q, al);
            const int w[4] = {(int)v.x, (int)v.y, (int)v.z, (int)v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) id[4 * q + j] = (w[j] & ~255) ? -1 : w[j];
        }
    }
    static __device__ __forceinline__ int one(const int32_t* p) { const int v = *p; return (v & ~255) ? -1 : v; }
};

// presence: uint32 [9], zeroed before the launch: bit (id & 31) of word (id >> 5) for every id of the map, word 8 != 0 when a label lies
// outside 0..255. Every workgroup collects its labels in an LDS bitmap and ORs the nonzero words into the device words at its end.
template <typename T>
__global__ __launch_bounds__(NT) void label_ids_kernel(const T* __restrict__ map, long n, uint32_t* __restrict__ presence) {
    __shared__ uint32_t bits[MG_MATTE_PRESENCE_WORDS];
    if (threadIdx.x < MG_MATTE_PRESENCE_WORDS) bits[threadIdx.x] = 0u;
    __syncthreads();
    const bool al = is16(map);
    const long groups = (n + GP - 1) / GP;
    int last = -2;                                               // a label map is piecewise constant: one LDS atomic per change, not per pixel
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long i0 = grp * GP;
        int id[GP];
        int cnt = GP;
        if (i0 + GP <= n) {
            Labels<T>::load(map + i0, al, id);
        } else {
            cnt = (int)(n - i0);
#pragma unroll
            for (int j = 0; j < GP; ++j) id[j] = j < cnt ? Labels<T>::one(map + i0 + j) : last;
        }
#pragma unroll
        for (int j = 0; j < GP; ++j) {
            if (j < cnt && id[j] != last) {
                last = id[j];
                if (last < 0) atomicOr(&bits[8], 1u);
                else atomicOr(&bits[last >> 5], 1u << (last & 31));
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < MG_MATTE_PRESENCE_WORDS && bits[threadIdx.x] != 0u) atomicOr(&presence[threadIdx.x], bits[threadIdx.x]);
}

struct IdList { uint8_t id[256]; };

// planes [n_ids][n]: 255 where the map equals ids[k], else 0. A lane reads its 16 labels once and writes 16 bytes per id.
template <typename T>
__global__ __launch_bounds__(NT) void label_planes_kernel(const T* __restrict__ map, long n, IdList ids, int n_ids, uint8_t* __restrict__ planes) {
    const bool al = is16(map);
    const long groups = (n + GP - 1) / GP;
    for (long grp = (long)blockIdx.x * NT + threadIdx.x; grp < groups; grp += (long)gridDim.x * NT) {
        const long i0 = grp * GP;
        if (i0 + GP <= n) {
            int id[GP];
            Labels<T>::load(map + i0, al, id);
            for (int k = 0; k < n_ids; ++k) {
                const int want = ids.id[k];
                uint32_t w[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    w[q] = (id[4 * q] == want ? 0xffu : 0u) | (id[4 * q + 1] == want ? 0xff00u : 0u) | (id[4 * q + 2] == want ? 0xff0000u : 0u) |
                           (id[4 * q + 3] == want ? 0xff000000u : 0u);
                uint8_t* d = planes + (long)k * n + i0;
                st16(d, make_uint4(w[0], w[1], w[2], w[3]), is16(d));
            }
        } else {
            for (long i = i0; i < n; ++i) {
                const int v = Labels<T>::one(map + i);
                for (int k = 0; k < n_ids; ++k) planes[(long)k * n + i] = v == (int)ids.id[k] ? 255 : 0;
            }
        }
    }
}

unsigned grid_of(long groups) {
    long blocks = (groups + NT - 1) / NT;
    if (blocks < 1) blocks = 1;
    if (blocks > MG_MATTE_MAX_BLOCKS) blocks = MG_MATTE_MAX_BLOCKS;
    return (unsigned)blocks;
}
}  // namespace

extern "C" int mg_matte_composite(const float* alpha, long frames, int P, int Hin, int Win, int crop_h, int crop_w, int H, int W, int snap,
                                  const uint8_t* frames_u8, const uint8_t* bg_image, long bg_frames, int bg_r, int bg_g, int bg_b, uint8_t* out,
                                  float* alpha_out, void* stream) {
    if (!alpha || !frames_u8 || !out || frames < 0 || P < 0) return -2;
    if (Hin <= 0 || Win <= 0 || H <= 0 || W <= 0 || crop_h <= 0 || crop_w <= 0 || crop_h > Hin || crop_w > Win) return -2;
    if ((long)Hin * Win > 0x7fffffffL || (long)H * W > 0x7fffffffL / 3) return -2;
    if (((uintptr_t)alpha & 3) || ((uintptr_t)alpha_out & 3)) return -2;
    if (bg_image ? (bg_frames != 1 && bg_frames != frames) : ((bg_r | bg_g | bg_b) & ~255)) return -2;
    if (frames == 0 || P == 0) return 0;
    if (frames > 65535) return -3;
    Geo g;
    g.Hin = Hin; g.Win = Win; g.Hc = crop_h; g.Wc = crop_w; g.H = H; g.W = W;
    g.sy = H > 1 ? (float)(crop_h - 1) / (float)(H - 1) : 0.f;
    g.sx = W > 1 ? (float)(crop_w - 1) / (float)(W - 1) : 0.f;
    g.snap = snap != 0;
    g.identity = H == crop_h && W == crop_w;
    const long npix = (long)H * W;
    const dim3 grid(grid_of((npix + GP - 1) / GP), (unsigned)frames);
    const uint32_t rgb = (uint32_t)bg_r | (uint32_t)bg_g << 8 | (uint32_t)bg_b << 16;
    if (bg_image)
        hipLaunchKernelGGL(composite_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, alpha, frames_u8, bg_image,
                           bg_frames == 1 ? 0L : npix * 3, 0u, P, g, out, alpha_out);
    else
        hipLaunchKernelGGL(composite_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, alpha, frames_u8, (const uint8_t*)nullptr, 0L, rgb, P, g,
                           out, alpha_out);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_matte_overlay(const uint8_t* frames_u8, const uint8_t* masks, long frames, int H, int W, int r, int g, int b, float alpha,
                                uint8_t* out, void* stream) {
    if (!frames_u8 || !masks || !out || frames < 0 || H <= 0 || W <= 0 || ((r | g | b) & ~255) || !(alpha >= 0.f && alpha <= 1.f)) return -2;
    if ((long)H * W > 0x7fffffffL / 3) return -2;
    if (frames == 0) return 0;
    const long npix = frames * H * W;
    hipLaunchKernelGGL(overlay_kernel, dim3(grid_of((npix + GP - 1) / GP)), dim3(NT), 0, (hipStream_t)stream, frames_u8, masks, npix,
                       (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16, alpha, out);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_matte_label_ids(const void* map, int elem_bytes, long n, uint32_t* presence, void* stream) {
    if (!map || !presence || n < 0 || (elem_bytes != 1 && elem_bytes != 4) || ((uintptr_t)map & (elem_bytes - 1)) || ((uintptr_t)presence & 3)) return -2;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mg_zero_words_kernel, dim3(1), dim3(64), 0, st, presence, (long)MG_MATTE_PRESENCE_WORDS);
    MG_CHECK_LAUNCH();
    if (n == 0) return 0;
    const unsigned grid = grid_of((n + GP - 1) / GP);
    if (elem_bytes == 1) hipLaunchKernelGGL(label_ids_kernel<uint8_t>, dim3(grid), dim3(NT), 0, st, (const uint8_t*)map, n, presence);
    else hipLaunchKernelGGL(label_ids_kernel<int32_t>, dim3(grid), dim3(NT), 0, st, (const int32_t*)map, n, presence);
    MG_CHECK_LAUNCH();
    return 0;
}

extern "C" int mg_matte_label_planes(const void* map, int elem_bytes, long n, const uint8_t* ids, int n_ids, uint8_t* planes, void* stream) {
    if (!map || n < 0 || n_ids < 0 || n_ids > 256 || (elem_bytes != 1 && elem_bytes != 4) || ((uintptr_t)map & (elem_bytes - 1))) return -2;
    if (n_ids > 0 && (!ids || !planes)) return -2;
    if (n == 0 || n_ids == 0) return 0;
    IdList list;
    for (int k = 0; k < 256; ++k) list.id[k] = k < n_ids ? ids[k] : 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = grid_of((n + GP - 1) / GP);
    if (elem_bytes == 1) hipLaunchKernelGGL(label_planes_kernel<uint8_t>, dim3(grid), dim3(NT), 0, st, (const uint8_t*)map, n, list, n_ids, planes);
    else hipLaunchKernelGGL(label_planes_kernel<int32_t>, dim3(grid), dim3(NT), 0, st, (const int32_t*)map, n, list, n_ids, planes);
    MG_CHECK_LAUNCH();
    return 0;
}
