// wave_probe_sweeps.hip -- TEST HARNESS ONLY: the 39- and 33-wide sweep instantiations of the wave-routine probe, in a translation
// unit of their own (they are most of the probe's device compile time; the namespace is renamed so that both units link).
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#define dwbc dwbc_wps
#include "wave_probe_body.h"
#undef dwbc

extern "C" const char *wave_probe_run_sweep(int kind, const void *args, int threads) {
    using namespace dwbc_wps;
    const WpArgs &a = *static_cast<const WpArgs *>(args);
    switch (kind) {
    case 0: return wp_run<WpSweep<0>>(a, threads);
    case 1: return wp_run<WpSweep<1>>(a, threads);
    case 2: return wp_run<WpSweep<2>>(a, threads);
    case 3: return wp_run<WpSweep<3>>(a, threads);
    case 4: return wp_run<WpSweep<4>>(a, threads);
    }
    return "sweep kind out of range";
}
