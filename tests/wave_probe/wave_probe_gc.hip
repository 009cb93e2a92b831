// wave_probe_gc.hip -- TEST HARNESS ONLY: the probe's instantiations of the general-contact kernel's routines (gj_inverse_rows,
// spd_inverse_reg, spd_inverse_scaled, mmg of dwbc_cycle_gc.h) and of pinv_cod_small / qr_small, contact_gram and wrench_maps (dwbc_cycle2.h), in a translation
// unit of their own: the 39- and 33-wide register sweeps compile beside the others (the namespace is renamed so that the units link).
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#define dwbc dwbc_wpg
#include "wave_probe_body.h"
#undef dwbc

// kind: the order of the WP_GC rows of wave_probe.hip
extern "C" const char *wave_probe_run_gc(int kind, const void *args, int threads) {
    using namespace dwbc_wpg;
    const WpArgs &a = *static_cast<const WpArgs *>(args);
    switch (kind) {
    case 0: return wp_run<WpPinvCod>(a, threads);
    case 1: return wp_run<WpGjRows<6>>(a, threads);
    case 2: return wp_run<WpGjRows<12>>(a, threads);
    case 3: return wp_run<WpGjRows<18>>(a, threads);
    case 4: return wp_run<WpSpdReg<39, true>>(a, threads);
    case 5: return wp_run<WpSpdReg<33, true>>(a, threads);
    case 6: return wp_run<WpSpdReg<33, false>>(a, threads);
    case 7: return wp_run<WpSpdScaled>(a, threads);
    case 8: return wp_run<WpMmg<12, 39, 39, 0>>(a, threads);
    case 9: return wp_run<WpMmg<12, 12, 39, 1>>(a, threads);
    case 10: return wp_run<WpMmg<33, 12, 12, 2>>(a, threads);
    case 11: return wp_run<WpMmg<12, 33, 12, 0>>(a, threads);
    case 12: return wp_run<WpGram<39>>(a, threads);
    case 13: return wp_run<WpGram<37>>(a, threads);
    case 14: return wp_run<WpGram<23>>(a, threads);
    case 15: return wp_run<WpGram<24>>(a, threads);
    case 16: return wp_run<WpGram<50>>(a, threads);
    case 17: return wp_run<WpWrench<39>>(a, threads);
    case 18: return wp_run<WpWrench<37>>(a, threads);
    case 19: return wp_run<WpWrench<23>>(a, threads);
    case 20: return wp_run<WpWrench<24>>(a, threads);
    case 21: return wp_run<WpWrench<50>>(a, threads);
    }
    return "general-contact kind out of range";
}
