// dwbc_kernels_task_qp.hip -- the built-in instantiations of the single-level task-QP kernel (dwbc_task_qp.h; dwbc_kernels.h holds the entry
// point and the row macro) in a translation unit of their own, as dwbc_kernels_task_space.hip is for the task-space kernel: TOCABI's size on
// its constant tree and on any tree.  dwbc_capi.hip takes the rows from dwbc_task_qp_rows() and launches them like its own; no kernel pack
// carries the kernel.  Kept apart so that the device code of every other kernel does not depend on this one.
#define DWBC_NO_BUILTIN_ROWS
#include "dwbc_kernels.h"

using namespace dwbc;

namespace {
const dwbc_plan::Row kTaskQpRows[] = {DWBC_ROW_TASK_QP(39, 34, TopoTocabi, 1) DWBC_ROW_TASK_QP(39, 34, TopoGeneric, 0)};
}

extern "C" const dwbc_plan::Row *dwbc_task_qp_rows(int *count) {
    *count = (int)(sizeof(kTaskQpRows) / sizeof(kTaskQpRows[0]));
    return kTaskQpRows;
}
