// wave_probe_f32.hip -- TEST HARNESS ONLY: the fp32 forms of the wave-routine probe (cross-lane primitives, fast_rcp / fast_rsqrt),
// in a translation unit of its own with the namespace renamed, as libdwbc_amd/csrc/dwbc_kernels_f32.hip builds the fp32 kernels.
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#define DWBC_REAL float
#define WAVE_PROBE_F32 1
#define dwbc dwbc_f32
#include "wave_probe_body.h"
#undef dwbc

extern "C" const char *wave_probe_run_f32(int which, const void *args, int threads) {
    using namespace dwbc_f32;
    const WpArgs &a = *static_cast<const WpArgs *>(args);
    if (which == 0) return wp_run<WpLanes>(a, threads);
    if (which == 1) return wp_run<WpMath>(a, threads);
    return "fp32 form out of range";
}
