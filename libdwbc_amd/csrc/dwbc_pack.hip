// dwbc_pack.hip -- the fused cycle kernels for ONE model size other than TOCABI's, as a loadable pack:
//   hipcc ... -DDWBC_PACK_N=<system dof> -DDWBC_PACK_NB=<bodies> -shared -o ../libdwbc_pack_<N>_<NB>.so dwbc_pack.hip
// (`make pack N=.. NB=..`; libdwbc_amd.build_pack(model) from Python).  The reference is model-generic (any URDF RBDL reads:
// src/dwbc.cpp:140-277, tests/dof_test/*.urdf); here the kernels keep their matrices in registers, so the sizes are template
// arguments and each (N, NB) is compiled once.  TopoGeneric build (dense A^-1 sweep), fp64, full-model cycle, the redistribution
// of a caller-supplied torque, gravity compensation, the dynamics of UpdateKinematics, the contact space of CalcContactConstraint and the task space of CalcTaskSpace; the reduced (centroidal) path is laid out for TOCABI's tree and is not part of a pack.  dwbc_batch_create() dlopens the pack of the
// loaded model's size from the directory of libdwbc_hip.so (or $DWBC_PACK_DIR).
#ifndef DWBC_PACK_N
#error "compile with -DDWBC_PACK_N=<system dof> -DDWBC_PACK_NB=<bodies>"
#endif
#include <vector>

#include "dwbc_kernels.h"

using namespace dwbc;

static_assert(DWBC_PACK_N == DWBC_PACK_NB + 5, "floating base (6 dof) + one revolute joint per further body");
static_assert(DWBC_PACK_N <= 50, "one lane per column, and the wave QP keeps (N - 6) + 20 rows on 64 lanes");
static_assert(DWBC_PACK_NB <= kMaxBodies, "body table");

// with -DDWBC_PACK_PARENTS=... the pack is built for that one kinematic tree (TopoPack, dwbc_topo.h: tree-sparse A^-1 sweep, compile-time
// round counts) and is only used for a model with exactly that parent table; without it, for any tree of the size (TopoGeneric)
#ifdef DWBC_PACK_PARENTS
#define DWBC_PACK_TOPO TopoPack
#define DWBC_PACK_KIND 2
#else
#define DWBC_PACK_TOPO TopoGeneric
#define DWBC_PACK_KIND 0
#endif
#define DWBC_PACK_ROWS(NLV)                                                                  \
    DWBC_ROWS_V2(DWBC_PACK_N, DWBC_PACK_NB, NLV, DWBC_PACK_TOPO, DWBC_PACK_KIND) \
    DWBC_ROW_LEAN(DWBC_PACK_N, DWBC_PACK_NB, NLV, DWBC_PACK_TOPO, DWBC_PACK_KIND)
static const dwbc_plan::Row kPack[] = {
#ifdef DWBC_PACK_ONLY_NLV  // development: one level count only (a quarter of the compile time)
    DWBC_PACK_ROWS(DWBC_PACK_ONLY_NLV)
#else
    DWBC_PACK_ROWS(1) DWBC_PACK_ROWS(2) DWBC_PACK_ROWS(3) DWBC_PACK_ROWS(4)
#endif
// the general-contact kernel (dwbc_cycle_gc.h: up to three simultaneously active contacts) of this model size, when its QP rows fit one
// per lane ((N - 6) torque rows + 30 cone rows <= 64)
#if (DWBC_PACK_N - 6 + 10 * 3) <= 64
    DWBC_ROW_GC(DWBC_PACK_N, DWBC_PACK_NB, 6, 0u)
#endif
// redistribution of a caller-supplied torque (dwbc_redistribute.h) of this model size and tree
    DWBC_ROW_REDIST(DWBC_PACK_N, DWBC_PACK_NB, DWBC_PACK_TOPO, DWBC_PACK_KIND)
// gravity compensation, alone or before that redistribution (dwbc_redistribute.h, GRAV = true)
    DWBC_ROW_GRAVCOMP(DWBC_PACK_N, DWBC_PACK_NB, DWBC_PACK_TOPO, DWBC_PACK_KIND)
// the dynamics half of UpdateKinematics on its own (dwbc_dynamics.h)
    DWBC_ROW_DYNAMICS(DWBC_PACK_N, DWBC_PACK_NB, DWBC_PACK_TOPO, DWBC_PACK_KIND)
// SetContact + CalcContactConstraint on their own (dwbc_contact_space.h)
    DWBC_ROW_CONTACT_SPACE(DWBC_PACK_N, DWBC_PACK_NB, DWBC_PACK_TOPO, DWBC_PACK_KIND)
};
// SetTaskSpace + CalcTaskSpace on their own (dwbc_task_space.h): the pack's row comes from a translation unit of its own
// (dwbc_pack_task_space.hip, linked into the same file), as the built-in ones do -- instantiated beside them it changed the code objects of
// the pack's cycle, redistribution, gravity-compensation and contact-space kernels
extern "C" const dwbc_plan::Row *dwbc_pack_task_space_rows(int *count);

#ifdef DWBC_PACK_PARENTS
// the tree this pack was compiled for: the loader compares it with the model's
extern "C" const int *dwbc_pack_parents(int *nb) {
    *nb = TopoPack::nb;
    return TopoPack::parent;
}
#endif
extern "C" const dwbc_plan::Row *dwbc_pack_table(int *count, unsigned *abi_tag) {
    static const std::vector<dwbc_plan::Row> all = [] {  // the rows of this translation unit, then the task-space kernel's
        std::vector<dwbc_plan::Row> v(kPack, kPack + sizeof(kPack) / sizeof(kPack[0]));
        int n = 0;
        const dwbc_plan::Row *ts = dwbc_pack_task_space_rows(&n);
        v.insert(v.end(), ts, ts + n);
        return v;
    }();
    *count = (int)all.size();
    *abi_tag = kernel_abi_tag();
    return all.data();
}
