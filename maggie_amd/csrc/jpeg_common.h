// What the JPEG sources share: jpegdec.hip, jpegprog.hip, jpegenc.hip and photometric.hip. Included INSIDE each source's unnamed namespace, behind
//   include/maggie_hip.h, and therefore without an include guard: tests/csrc/*_host.cpp compile several of the sources into one program, each in
//   a namespace of its own, and every one of them needs its own copy. Nothing here becomes a device symbol (constants and inlined functions only),
//   so the code objects do not depend on where a piece is written.

// ---- the zig-zag order: the natural-order index of zig-zag position k. A macro and not a table, so that each source keeps its table under the
//   name its code object has always carried
#define MG_JPEG_ZIGZAG \
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// ---- libjpeg's JDCT_ISLOW, pinned to Pillow: CONST_BITS 13, PASS1_BITS 2
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633;
constexpr int F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995;
constexpr int F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jpeg_fdct_islow: FIRST = the row pass (outputs 0 and 4 times 4, the others descaled by 11), else the column pass (2 and 15)
template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = FIRST ? 11 : 15;
    d[0] = FIRST ? (tmp10 + tmp11) * 4 : descale(tmp10 + tmp11, 2);
    d[4] = FIRST ? (tmp10 - tmp11) * 4 : descale(tmp10 - tmp11, 2);
    int z1 = (tmp12 + tmp13) * F_0_541196100;
    d[2] = descale(z1 + tmp13 * F_0_765366865, n);
    d[6] = descale(z1 + tmp12 * (-F_1_847759065), n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    d[7] = descale(t4 + z1 + z3, n);
    d[5] = descale(t5 + z2 + z4, n);
    d[3] = descale(t6 + z2 + z3, n);
    d[1] = descale(t7 + z1 + z4, n);
}

// one pass of jpeg_idct_islow on dequantised values, descaled by N bits (11 for the columns, 18 for the rows)
template <int N>
__device__ __forceinline__ void idct8(int (&d)[8]) {
    int z1 = (d[2] + d[6]) * F_0_541196100;
    int tmp2 = z1 + d[6] * (-F_1_847759065), tmp3 = z1 + d[2] * F_0_765366865;
    int tmp0 = (d[0] + d[4]) * 8192, tmp1 = (d[0] - d[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
    z1 = tmp0 + tmp3;
    int z2 = tmp1 + tmp2, z3 = tmp0 + tmp2, z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    d[0] = descale(tmp10 + tmp3, N); d[7] = descale(tmp10 - tmp3, N);
    d[1] = descale(tmp11 + tmp2, N); d[6] = descale(tmp11 - tmp2, N);
    d[2] = descale(tmp12 + tmp1, N); d[5] = descale(tmp12 - tmp1, N);
    d[3] = descale(tmp13 + tmp0, N); d[4] = descale(tmp13 - tmp0, N);
}

// libjpeg's range-limit table behind the inverse transform, indexed with the descaled value masked to 10 bits: v + 128 for -128 <= v < 128,
// 255 up to 511, 0 from -512 on -- and, unlike a clamp, periodic beyond
__device__ __forceinline__ int range_limit(int v) {
    const int i = v & 1023;
    return i < 128 ? i + 128 : (i < 512 ? 255 : (i < 896 ? 0 : i - 896));
}

// ---- one Huffman table as the kernels read it, HT int32 words: look uint16[256] (len << 8 | symbol for codes of at most 8 bits, else 0), then
//   from word HT_MAXCODE maxcode[18] by code length (-1 = none), from HT_VALOFF valoff[18] (index of the length's first value minus its first
//   code), from HT_VALS vals uint8[256]
constexpr int HT_MAXCODE = 128, HT_VALOFF = HT_MAXCODE + 18, HT_VALS = HT_VALOFF + 18, HT = HT_VALS + 64;
static_assert(HT == 228, "four tables and the header words make MG_JPEGDEC_TAB_WORDS, two MG_JPEGPROG_SCAN_WORDS");

// ---- the six layouts (MG_JPEGDEC_420 ... MG_JPEGDEC_411): luma sampling (hs, vs) over (1, 1) Cb and Cr, or one component; the MCU grid of an
//   h x w frame; the row pitches of its planes in bytes. The planes of 4:2:0, 4:4:4 and grey are as wide as their blocks; those of 4:2:2, 4:4:0 and
//   4:1:1 are pitched so that the widest load of a lane of mg_jpeg_rgb_hv stays inside its row: luma to 16 bytes, 4:4:0 chroma (16 samples a
//   lane) too. Host side only: each source fills the struct its kernels take from this.
struct JpegLayout { int hs, vs, ncomp, bpm, mcux, mcuy, yp, cp; };

inline bool jpeg_layout(int layout, int h, int w, JpegLayout& g) {
    static const int HV[6][2] = {{2, 2}, {1, 1}, {1, 1}, {2, 1}, {1, 2}, {4, 1}};              // by MG_JPEGDEC_420, _444, _GREY, _422, _440, _411
    if (layout < MG_JPEGDEC_420 || layout > MG_JPEGDEC_411) return false;
    g.hs = HV[layout][0]; g.vs = HV[layout][1];
    g.ncomp = layout == MG_JPEGDEC_GREY ? 1 : 3;
    g.bpm = g.hs * g.vs + g.ncomp - 1;
    g.mcux = (w + 8 * g.hs - 1) / (8 * g.hs);
    g.mcuy = (h + 8 * g.vs - 1) / (8 * g.vs);
    g.yp = g.mcux * 8 * g.hs; g.cp = g.mcux * 8;
    if (layout >= MG_JPEGDEC_422) { g.yp = (g.yp + 15) & ~15; if (g.vs == 2) g.cp = (g.cp + 15) & ~15; }
    return true;
}
inline bool jpeg_bad_size(long frames, int h, int w) { return frames < 0 || h <= 0 || w <= 0 || h > MG_JPEG_MAX_SIDE || w > MG_JPEG_MAX_SIDE; }
