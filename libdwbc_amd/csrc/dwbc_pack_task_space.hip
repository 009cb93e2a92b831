// dwbc_pack_task_space.hip -- the task-space kernel (dwbc_task_space.h) of a kernel pack's model size and tree, in a translation unit of
// its own beside dwbc_pack.hip (same -D flags, linked into the same libdwbc_pack_<N>_<NB>.so): the pack's other kernels are then compiled in
// a module that does not hold this one, and keep the code objects they had.  dwbc_pack.hip appends the row to the table it hands out.
#ifndef DWBC_PACK_N
#error "compile with -DDWBC_PACK_N=<system dof> -DDWBC_PACK_NB=<bodies>"
#endif
#include "dwbc_kernels.h"

using namespace dwbc;

#ifdef DWBC_PACK_PARENTS
#define DWBC_PACK_TOPO TopoPack
#define DWBC_PACK_KIND 2
#else
#define DWBC_PACK_TOPO TopoGeneric
#define DWBC_PACK_KIND 0
#endif
static const dwbc_plan::Row kPackTaskSpace[] = {DWBC_ROW_TASK_SPACE(DWBC_PACK_N, DWBC_PACK_NB, DWBC_PACK_TOPO, DWBC_PACK_KIND)};

extern "C" const dwbc_plan::Row *dwbc_pack_task_space_rows(int *count) {
    *count = (int)(sizeof(kPackTaskSpace) / sizeof(kPackTaskSpace[0]));
    return kPackTaskSpace;
}
