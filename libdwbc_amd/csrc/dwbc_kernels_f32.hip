// dwbc_kernels_f32.hip -- the fp32 build of the fused cycle kernels (BASELINE config 5 names an fp32 path).  Same source as the
// fp64 product kernels (dwbc_kernels.h) with DWBC_REAL = float; the namespace is renamed so that both builds link into
// libdwbc_hip.so.  dwbc_capi.hip takes the rows of this build's launch table from dwbc_f32_rows() and launches them like its own.
#define DWBC_REAL float
#define DWBC_NO_PAIR_KERNEL
#define DWBC_NO_GC_KERNEL
#define DWBC_NO_REDIST_KERNEL
#define DWBC_NO_LINK_QUERY_KERNEL
#define DWBC_NO_DYNAMICS_KERNEL
#define DWBC_NO_CONTACT_SPACE_KERNEL
#define DWBC_NO_TASK_SPACE_KERNEL
#define dwbc dwbc_f32
#include "dwbc_kernels.h"
#undef dwbc

extern "C" const dwbc_plan::Row *dwbc_f32_rows(int *count) {
    *count = (int)(sizeof(dwbc_f32::kRows) / sizeof(dwbc_f32::kRows[0]));
    return dwbc_f32::kRows;
}
