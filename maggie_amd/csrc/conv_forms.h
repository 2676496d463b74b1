// Host-side record of the convolution kernel forms a public entry call launched (mg_conv_form_count / _name / mg_conv_last_forms in
// include/maggie_hip.h). A launch site stores ONE 64-bit word -- the packed template arguments of the kernel it is about to launch -- into a
// thread-local list; names are formatted only when a caller asks for them (conv_forms.hip). Nothing here reaches device code.
#pragma once
#include <stdint.h>

enum {
    MG_FF_H3 = 1,           // conv_halo3_kernel<TH, BN, NS, MODE, RES, XF, BNB>
    MG_FF_H3_SLAB,          // conv_halo3_slab_kernel<MODE, RES, XF>
    MG_FF_H3_PERSIST,       // conv_halo3_persist_kernel<TH, BN, NS, MODE, RES>
    MG_FF_HALO,             // igemm_fprop_halo_kernel<TH, BN, NS, MODE, BNB, XF>
    MG_FF_C8,               // igemm_fprop_c8_kernel<TH>
    MG_FF_ASYNC,            // igemm_fprop_async_kernel<BM, BN, KS, NS, MODE, BNB>
    MG_FF_ASYNC_MDEV,       // igemm_fprop_async_persistent_kernel<BM, BN, KS, NS, MODE>
    MG_FF_FPROP,            // igemm_fprop_kernel<BM, BN, KS, MODE, false, BNB> (MG_FORM_PHASED: the phase-major transposed walk)
    MG_FF_FPROP_MDEV,       // igemm_fprop_persistent_kernel<BM, BN, KS, MODE, XF>
    MG_FF_SPLIT,            // igemm_fprop_kernel<128, BN, 4, MODE, true>
    MG_FF_SPLIT_FINISH,     // splitk_finish_kernel
    MG_FF_WGRAD_C8,         // igemm_wgrad_c8_kernel
    MG_FF_WGRAD_GATHER9,    // igemm_wgrad_gather9_kernel<FM, XF>
    MG_FF_WGRAD_HALO,       // igemm_wgrad_halo_kernel<1, 1, XF>
    MG_FF_WGRAD,            // igemm_wgrad_kernel<TCO, TCI, MODE, XF>
    MG_FF_REDUCE,           // wgrad_reduce_kernel
    MG_FF_REDUCE_WAVE,      // wgrad_reduce_wave_kernel
    MG_FF_REDUCE_TILE,      // wgrad_reduce_tile_kernel
    MG_FF_REDUCE_BATCHED,   // wgrad_reduce_batched_kernel
    MG_FF_END
};
#define MG_FORM_NOMODE 7    /* the kernel is not templated on the mode */
#define MG_FORM_RES 1
#define MG_FORM_XF 2
#define MG_FORM_BNB 4
#define MG_FORM_PHASED 8

// byte 0 family | 1..4 the integer template arguments in their order | 5 mode | 6 flags
constexpr uint64_t mg_form_code(int fam, int a, int b, int c, int d, int mode, int flags) {
    return (uint64_t)(uint8_t)fam | (uint64_t)(uint8_t)a << 8 | (uint64_t)(uint8_t)b << 16 | (uint64_t)(uint8_t)c << 24 | (uint64_t)(uint8_t)d << 32 |
           (uint64_t)(uint8_t)mode << 40 | (uint64_t)(uint8_t)flags << 48;
}

// The halo3 tile forms (TH, BN, NS) and persistent ring forms: ONE list, expanded by dispatch_h3 (conv_halo3.hip) into its launch cases and by
// conv_forms.hip into the names -- a form added here cannot be launched without being listed.
#ifdef MG_H3_EXTRA_FORMS
#define MG_H3_TILE_FORMS(X) X(8, 64, 3) X(8, 64, 1) X(8, 32, 4) X(8, 32, 1) X(4, 32, 4) X(8, 64, 2) X(8, 32, 2) X(4, 64, 3)
#else
#define MG_H3_TILE_FORMS(X) X(8, 64, 3) X(8, 64, 1) X(8, 32, 4) X(8, 32, 1) X(4, 32, 4)
#endif
#define MG_H3_PERSIST_FORMS(X) X(8, 64, 3) X(8, 32, 4)

extern "C" __attribute__((visibility("hidden"))) void mg_conv_forms_clear(void);
extern "C" __attribute__((visibility("hidden"))) void mg_conv_forms_push(uint64_t code);

#define MG_FORM(fam, a, b, c, d, mode, flags) mg_conv_forms_push(mg_form_code(fam, a, b, c, d, mode, flags))
