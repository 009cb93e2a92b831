// dwbc_kernels_task_space.hip -- the built-in instantiations of the task-space kernel (dwbc_task_space.h; dwbc_kernels.h holds the entry
// point and the row macro) in a translation unit of their own: TOCABI's size on its constant tree and on any tree.  dwbc_capi.hip takes the
// rows from dwbc_task_space_rows() as it takes the fp32 build's, and launches them like its own; the kernel packs emit theirs themselves
// (dwbc_pack.hip).  Kept apart from dwbc_capi.hip so that the device code of the kernels compiled there does not depend on this one.
#define DWBC_NO_BUILTIN_ROWS
#include "dwbc_kernels.h"

using namespace dwbc;

namespace {
const dwbc_plan::Row kTaskSpaceRows[] = {DWBC_ROW_TASK_SPACE(39, 34, TopoTocabi, 1) DWBC_ROW_TASK_SPACE(39, 34, TopoGeneric, 0)};
}

extern "C" const dwbc_plan::Row *dwbc_task_space_rows(int *count) {
    *count = (int)(sizeof(kTaskSpaceRows) / sizeof(kTaskSpaceRows[0]));
    return kTaskSpaceRows;
}
