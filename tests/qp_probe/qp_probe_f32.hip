// qp_probe_f32.hip -- TEST HARNESS ONLY: the fp32 instantiation of the wave-QP probe, in a translation unit of its own with the
// namespace renamed, as libdwbc_amd/csrc/dwbc_kernels_f32.hip builds the fp32 kernels beside the fp64 ones.
#ifndef DWBC_HOST_EMU
#include <hip/hip_runtime.h>
#endif
#define DWBC_REAL float
#define dwbc dwbc_f32
#include "qp_probe_body.h"
#undef dwbc

extern "C" double qp_probe_scale_f32() { return (double)dwbc_f32::kQpScaleGI; }

extern "C" const char *qp_probe_run_f32(const void *args, int threads) {
    return dwbc_f32::qp_probe_run<1, 12, 12, 6>(*static_cast<const dwbc_f32::QpProbeArgs *>(args), threads);
}
