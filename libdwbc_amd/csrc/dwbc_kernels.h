// dwbc_kernels.h -- __global__ entry points of the fused cycle and the table of instantiations.  Included by dwbc_capi.hip
// (DWBC_REAL = double, the product path) and by dwbc_kernels_f32.hip (DWBC_REAL = float with the namespace renamed to
// dwbc_f32): the same source in both arithmetic types, each emitting its rows of the launch table (dwbc_launch_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "dwbc_launch_plan.h"
#include "dwbc_reduced.h"
#include "dwbc_cycle2p.h"
#include "dwbc_cycle_gc.h"
#include "dwbc_redistribute.h"
#include "dwbc_link_query.h"
#include "dwbc_dynamics.h"
#include "dwbc_contact_space.h"
#include "dwbc_task_space.h"
#include "dwbc_task_qp.h"

namespace dwbc {

// register-resident kernel (dwbc_cycle2.h): one workgroup (one 64-lane wavefront) per robot instance.  Two builds of the same body:
//   _v2   amdgpu_waves_per_eu(2): VGPR + AGPR <= 256, so a fifth workgroup of a CU (the LDS map allows 5 at <= 31 KB) can
//         share a SIMD -- the throughput build for batches larger than 4 instances per CU
//   _v2w  no register cap (one wave per SIMD): ~7 % shorter single-instance latency -- used while B <= 4 x CUs
#define DWBC_V2_BODY(COMPACT)                                                            \
    static_assert(NT == 64, "one wavefront per instance");                               \
    extern __shared__ __attribute__((aligned(16))) real_t lds[];                         \
    const int inst = blockIdx.x;                                                         \
    if (inst >= io.B) return;                                                            \
    Thr th{(int)threadIdx.x};                                                            \
    int *iL = reinterpret_cast<int *>(lds + V2Lds<N, NB, NLV, COMPACT>::type::total);    \
    cycle_instance_v2<N, NB, NLV, NT, EXTRAS, Topo, COMPACT>(th, su, io, inst, lds, iL);
// EXTRAS: see cycle_instance_v2 -- false = the lean build the launcher uses when no optional path is requested
// Topo: a constant kinematic tree (dwbc_topo.h) whose sparsity the A^-1 sweep uses, or TopoGeneric
// COMPACT: the 20 KB LDS map (Lds3, dwbc_cycle2.h) -- the lean capped build of a constant-tree model takes it: eight workgroups
// share a CU (two waves per SIMD) instead of five
template <int N, int NB, int NLV, bool COMPACT>
struct V2Lds { using type = typename std::conditional<COMPACT, Lds3<N, NB, NLV>, Lds2<N, NB, NLV>>::type; };
template <int N, int NB, int NLV, int NT, bool EXTRAS, class Topo, bool COMPACT = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_cycle_kernel_v2(const Setup su, const BatchIO io) {
    DWBC_V2_BODY(COMPACT)
}
#ifndef DWBC_WIDE_ATTR
#define DWBC_WIDE_ATTR
#endif
template <int N, int NB, int NLV, int NT, bool EXTRAS, class Topo>
__global__ __launch_bounds__(NT) DWBC_WIDE_ATTR void dwbc_cycle_kernel_v2w(const Setup su, const BatchIO io) {
    DWBC_V2_BODY(false)
}

// two wavefronts per instance (dwbc_cycle2p.h): the lean cycle of batches of at most one instance per SIMD, side chains on a helper wave.
// roles: wave 0 is the main wave, except in the workgroups whose index has bit io.pair_swap_bit set (see dwbc_batch launch: the
// waves of consecutive workgroups of a CU land on SIMDs round-robin, and the main waves should not share one)
template <int N, int NB, int NLV, class Topo>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_cycle_kernel_v2p(const Setup su, const BatchIO io) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    int wave = (int)(threadIdx.x >> 6);
    if (io.pair_swap_bit >= 0 && ((blockIdx.x >> io.pair_swap_bit) & 1)) wave ^= 1;
    Thr th{(int)(threadIdx.x & 63u)};
    cycle_instance_v2p<N, NB, NLV, 64, Topo>(wave, th, su, io, inst, lds);
}

// up to three simultaneously active contacts (dwbc_cycle_gc.h): the general statement of the cycle, matrices in LDS (80 KB: two
// workgroups per CU), any number of task levels -- for batches that opt in with dwbc_batch_set_max_active_contacts(b, 3)
// TG = 12: the same cycle sized for task levels of up to 12 dof (two 6D links on one level -- both hands, reference
// tests/sp_test/regulation_test.cpp:90-91): QPs of up to 24 variables, 105 KB of LDS, one workgroup per CU
constexpr int kGcContacts = 3;
template <int N, int NB, int NT, int TG = kMaxTaskDof>
__global__ __launch_bounds__(NT) void dwbc_cycle_kernel_gc(const Setup su, const BatchIO io) {
    static_assert(NT == 64, "one wavefront per instance");
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    cycle_instance_gc<N, NB, kGcContacts, NT, TG>(th, su, io, inst, lds);
}

// reduced (centroidal) dynamics model, dwbc_reduced.h: Reduced* call sequence of reference include/dwbc.h:411-416
template <int N, int NB, int NLV, int NT, class Topo>
__global__ __launch_bounds__(NT) void dwbc_cycle_kernel_reduced(const Setup su, const BatchIO io) {
    static_assert(NT == 64, "one wavefront per instance");
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    int *iL = reinterpret_cast<int *>(lds + LdsR<N, NB, NLV>::rtotal);
    cycle_instance_reduced<N, NB, NLV, NT, Topo>(th, su, io, inst, lds, iL);
}

// contact redistribution of a caller-supplied torque (dwbc_redistribute.h): the front half of the cycle and one six-variable QP on the
// compact map's footprint (LdsRd: 12.9 KB at 23 dof, 20.4 KB at 39, 26.8 KB at 50) -- register-capped like `_v2`, up to eight workgroups
// per CU; no instantiation spills to scratch under the cap, the 43-dof TopoDense route included, so there is no uncapped variant
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_redistribute_kernel(const Setup su, const BatchIO io, const RedistIO rio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    redistribute_instance<N, NB, 64, Topo>(th, su, io, rio, inst, lds);
}

// gravity compensation, alone or with the redistribution of a command on top of it (dwbc_redistribute.h, GRAV = true): the redistribution
// kernel's stages with torque_grav_ formed behind P_C, on the same map (LdsGc adds tenants, no bytes) and under the same register cap.  One
// instantiation serves both forms: without GravIO::tau_in NwJw and the QP are skipped by a wave-uniform branch
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_gravcomp_kernel(const Setup su, const BatchIO io, const GravIO gio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    const RedistIO rio{gio.tau_in, gio.rd_tau, gio.rd_cf, gio.rd_wrench, gio.rd_status};
    redistribute_instance<N, NB, 64, Topo, true>(th, su, io, rio, inst, lds, &gio);
}

// link poses, velocities and Jacobians in a launch of their own (dwbc_link_query.h): forward kinematics and, for the COM link, the six
// base rows of A -- 13 KB of LDS, no register cap; the tree is read at run time
template <int N, int NB>
__global__ __launch_bounds__(64) void dwbc_link_query_kernel(const BatchIO io, const LinkQueryIO lq) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    link_query_instance<N, NB, 64>(th, io, lq, inst, lds);
}

// the dynamics half of UpdateKinematics in a launch of its own (dwbc_dynamics.h): stage 0 and, each behind a wave-uniform branch on
// DynIO::mask, the centroidal block, the A^-1 sweep and the RNEA of B_ -- 15 KB of LDS at TOCABI's size (LdsDyn), register-capped like the
// other lean kernels: eight workgroups per CU
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_dynamics_kernel(const Setup su, const BatchIO io, const DynIO dio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    dynamics_instance<N, NB, 64, Topo>(th, su, io, dio, inst, lds);
}

// SetContact + CalcContactConstraint in a launch of its own (dwbc_contact_space.h): stage 0, the contact stage and, each behind a
// wave-uniform branch on CsIO::mask, N_C, A^-1 N_c / W, the NwJw closed form and the W^+ sweep -- the redistribution kernel's LDS map,
// register-capped like the other lean kernels: eight workgroups per CU
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_contact_space_kernel(const Setup su, const BatchIO io, const CsIO cio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    contact_space_instance<N, NB, 64, Topo>(th, su, io, cio, inst, lds);
}

// SetTaskSpace + CalcTaskSpace in a launch of their own (dwbc_task_space.h): the contact-space kernel's front and, per task level and each
// behind a wave-uniform branch on TsIO::mask, J_task, Lambda_task, J_kt and Null_task -- LdsTs (38 KB at TOCABI's size: four workgroups per
// CU), register-capped like the other lean kernels
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_task_space_kernel(const Setup su, const BatchIO io, const TsIO tio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    task_space_instance<N, NB, 64, Topo>(th, su, io, tio, inst, lds);
}

// CalcSingleTaskTorqueWithQP for one task level in a launch of its own (dwbc_task_qp.h): the task-space kernel's front for that level, the
// operands of the QP rows and the cycle's row fill and solver -- LdsTq (37 KB at TOCABI's size: four workgroups per CU), register-capped like
// the other lean kernels
template <int N, int NB, class Topo>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void dwbc_task_qp_kernel(const Setup su, const BatchIO io, const TqIO qio) {
    extern __shared__ __attribute__((aligned(16))) real_t lds[];
    const int inst = blockIdx.x;
    if (inst >= io.B) return;
    Thr th{(int)threadIdx.x};
    task_qp_instance<N, NB, 64, Topo>(th, su, io, qio, inst, lds);
}

#define DWBC_NT 64  // threads of the one-wave kernels, as a literal: the rows below spell it into the kernel names
constexpr int kNT = DWBC_NT;
static_assert(kMaxTaskDof == 6 && kMaxTaskDofWide == 12, "the TG arguments of the general-contact rows below");
// dwbc_capi.hip fills one BatchIO for the kernels of both arithmetic types: the members that differ are pointers
static_assert(sizeof(BatchIO) == 8 + 15 * sizeof(void *) + 4 * sizeof(int) && offsetof(BatchIO, body) == 8 + 12 * sizeof(void *),
              "BatchIO layouts of the two builds must match");

// ---- the launch table (dwbc_launch_plan.h): one row per launchable kernel.  DWBC_ROW instantiates KERNEL<template arguments> and
// spells the same tokens into the row's name, so the name reported for a launch is the kernel's own (the fp32 build's rename of
// `dwbc` reaches both).  A defaulted COMPACT = false is left out, as the names always were.
namespace lp = dwbc_plan;
#define DWBC_STR_(...) #__VA_ARGS__
#define DWBC_STR(...) DWBC_STR_(__VA_ARGS__)
// a DWBC_INST_MODEL build (dwbc_kernels_im.h) marks every row it emits: the planner hands such a row to a batch with a per-instance body
// table and to no other
#ifdef DWBC_INST_MODEL
#define DWBC_ROW_BUILD_FLAVOUR lp::kInstModel
#else
#define DWBC_ROW_BUILD_FLAVOUR 0u
#endif
#define DWBC_ROW(N, NB, NLV, TOPO_KIND, KIND, FLAVOUR, LDS, THREADS, KERNEL, ...)                                           \
    lp::Row{N, NB, NLV, TOPO_KIND, kF32 ? lp::kFloat : lp::kDouble, lp::KIND, (FLAVOUR) | DWBC_ROW_BUILD_FLAVOUR,           \
            reinterpret_cast<const void *>(&dwbc::KERNEL<__VA_ARGS__>), (int)LDS, THREADS, DWBC_STR(dwbc::KERNEL), DWBC_STR(__VA_ARGS__)}
// capped extras, wide extras and wide lean build of one model size, level count and tree (TK: Row::topo of TOPO); the capped lean
// build is laid out on the compact map (Lds3) for TOCABI's tree and on Lds2 in the packs
#define DWBC_ROWS_V2(N, NB, NLV, TOPO, TK)                                                                                                       \
    DWBC_ROW(N, NB, NLV, TK, kCycle, 0u, (Lds2<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2, N, NB, NLV, DWBC_NT, true, dwbc::TOPO),       \
    DWBC_ROW(N, NB, NLV, TK, kCycle, lp::kWide, (Lds2<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2w, N, NB, NLV, DWBC_NT, true, dwbc::TOPO), \
    DWBC_ROW(N, NB, NLV, TK, kCycle, lp::kWide | lp::kLean, (Lds2<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2w, N, NB, NLV, DWBC_NT, false, dwbc::TOPO),
#define DWBC_ROW_LEAN(N, NB, NLV, TOPO, TK) \
    DWBC_ROW(N, NB, NLV, TK, kCycle, lp::kLean, (Lds2<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2, N, NB, NLV, DWBC_NT, false, dwbc::TOPO),
#define DWBC_ROW_LEAN_COMPACT(N, NB, NLV, TOPO, TK) \
    DWBC_ROW(N, NB, NLV, TK, kCycle, lp::kLean | lp::kCompact, (Lds3<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2, N, NB, NLV, DWBC_NT, false, dwbc::TOPO, true),
#define DWBC_ROW_REDUCED(N, NB, NLV, TOPO, TK) \
    DWBC_ROW(N, NB, NLV, TK, kReduced, 0u, (LdsR<N, NB, NLV>::total_bytes), kNT, dwbc_cycle_kernel_reduced, N, NB, NLV, DWBC_NT, dwbc::TOPO),
// any tree, any number of levels.  DWBC_NO_GC_KERNEL: a build without the general-contact kernel (fp32)
#ifdef DWBC_NO_GC_KERNEL
#define DWBC_ROW_GC(N, NB, TG, FLAVOUR)
#else
#define DWBC_ROW_GC(N, NB, TG, FLAVOUR) \
    DWBC_ROW(N, NB, 0, 0, kGc, FLAVOUR, (LdsG<N, NB, kGcContacts, TG>::total_bytes), kNT, dwbc_cycle_kernel_gc, N, NB, DWBC_NT, TG),
#endif
// the two-wave kernel exists in the fp64 build (DWBC_NO_PAIR_KERNEL: fp32), for one and two task levels (three levels no longer fit
// four workgroups per CU)
#ifdef DWBC_NO_PAIR_KERNEL
#define DWBC_ROW_PAIR(NLV)
#else
#define DWBC_ROW_PAIR(NLV) \
    DWBC_ROW(39, 34, NLV, 1, kCycle, lp::kLean | lp::kTwoWave, (Lds4<39, 34, NLV>::total_bytes), 2 * kNT, dwbc_cycle_kernel_v2p, 39, 34, NLV, dwbc::TopoTocabi),
#endif
// the redistribution kernel: fp64 (DWBC_NO_REDIST_KERNEL: fp32), for a constant tree or any tree of the size; every kernel pack carries its own
#ifdef DWBC_NO_REDIST_KERNEL
#define DWBC_ROW_REDIST(N, NB, TOPO, TK)
#else
#define DWBC_ROW_REDIST(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kRedist, 0u, (LdsRd<N, NB>::total_bytes), kNT, dwbc_redistribute_kernel, N, NB, dwbc::TOPO),
#endif
// the gravity-compensation kernel: wherever the redistribution kernel is
#ifdef DWBC_NO_REDIST_KERNEL
#define DWBC_ROW_GRAVCOMP(N, NB, TOPO, TK)
#else
#define DWBC_ROW_GRAVCOMP(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kGravComp, 0u, (LdsGc<N, NB>::total_bytes), kNT, dwbc_gravcomp_kernel, N, NB, dwbc::TOPO),
#endif
// the link-query kernel: fp64, any tree of its size (DWBC_NO_LINK_QUERY_KERNEL: fp32); not part of a kernel pack
#ifdef DWBC_NO_LINK_QUERY_KERNEL
#define DWBC_ROW_LINK_QUERY(N, NB)
#else
#define DWBC_ROW_LINK_QUERY(N, NB) DWBC_ROW(N, NB, 0, 0, kLinkQuery, 0u, (LdsLq<N, NB>::total_bytes), kNT, dwbc_link_query_kernel, N, NB),
#endif
// the dynamics kernel: fp64 (DWBC_NO_DYNAMICS_KERNEL: fp32), for a constant tree or any tree of the size; every kernel pack carries its own
#ifdef DWBC_NO_DYNAMICS_KERNEL
#define DWBC_ROW_DYNAMICS(N, NB, TOPO, TK)
#else
#define DWBC_ROW_DYNAMICS(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kDynamics, 0u, (LdsDyn<N, NB>::total_bytes), kNT, dwbc_dynamics_kernel, N, NB, dwbc::TOPO),
#endif
// the contact-space kernel: fp64 (DWBC_NO_CONTACT_SPACE_KERNEL: fp32), for a constant tree or any tree of the size; every kernel pack carries its own
#ifdef DWBC_NO_CONTACT_SPACE_KERNEL
#define DWBC_ROW_CONTACT_SPACE(N, NB, TOPO, TK)
#else
#define DWBC_ROW_CONTACT_SPACE(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kContactSpace, 0u, (LdsCs<N, NB>::total_bytes), kNT, dwbc_contact_space_kernel, N, NB, dwbc::TOPO),
#endif
// the task-space kernel: fp64 (DWBC_NO_TASK_SPACE_KERNEL: fp32), for a constant tree or any tree of the size; every kernel pack carries its own
#ifdef DWBC_NO_TASK_SPACE_KERNEL
#define DWBC_ROW_TASK_SPACE(N, NB, TOPO, TK)
#else
#define DWBC_ROW_TASK_SPACE(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kTaskSpace, 0u, (LdsTs<N, NB>::total_bytes), kNT, dwbc_task_space_kernel, N, NB, dwbc::TOPO),
#endif
// the single-level task-QP kernel: fp64, for a constant tree or any tree of the size; built in only (dwbc_kernels_task_qp.hip), no kernel
// pack carries one
#define DWBC_ROW_TASK_QP(N, NB, TOPO, TK) \
    DWBC_ROW(N, NB, 0, TK, kTaskQp, 0u, (LdsTq<N, NB>::total_bytes), kNT, dwbc_task_qp_kernel, N, NB, dwbc::TOPO),
// instantiated model sizes (system dof, bodies).  TOCABI = (39, 34), the only model in BASELINE.json's configs: its four flavours
// and the reduced path use the constant tree; any other 34-body tree runs the TopoGeneric builds (capped extras flavour only).  Other
// model sizes come from kernel packs (dwbc_pack.hip: this header instantiated for one (N, NB), loaded by the C-ABI at model-load time).
#define DWBC_ROWS_TOCABI_TREE(NLV) \
    DWBC_ROWS_V2(39, 34, NLV, TopoTocabi, 1) DWBC_ROW_LEAN_COMPACT(39, 34, NLV, TopoTocabi, 1) DWBC_ROW_REDUCED(39, 34, NLV, TopoTocabi, 1)
#define DWBC_ROWS_TOCABI_ANY(NLV) \
    DWBC_ROW(39, 34, NLV, 0, kCycle, 0u, (Lds2<39, 34, NLV>::total_bytes), kNT, dwbc_cycle_kernel_v2, 39, 34, NLV, DWBC_NT, true, dwbc::TopoGeneric), \
    DWBC_ROW_REDUCED(39, 34, NLV, TopoGeneric, 0)
#if !defined(DWBC_PACK_N) && !defined(DWBC_NO_BUILTIN_ROWS)
const lp::Row kRows[] = {
#ifdef DWBC_EXPERIMENT
    // A/B build (make experiment VARIANT=.. XFLAGS=..): only the BASELINE config[1] instantiations, seconds to compile
    DWBC_ROWS_TOCABI_TREE(2) DWBC_ROW_PAIR(2)
#else
    DWBC_ROWS_TOCABI_TREE(1) DWBC_ROWS_TOCABI_TREE(2) DWBC_ROWS_TOCABI_TREE(3) DWBC_ROWS_TOCABI_TREE(4)
    DWBC_ROW_PAIR(1) DWBC_ROW_PAIR(2)
    DWBC_ROWS_TOCABI_ANY(1) DWBC_ROWS_TOCABI_ANY(2) DWBC_ROWS_TOCABI_ANY(3) DWBC_ROWS_TOCABI_ANY(4)
#endif
    DWBC_ROW_GC(39, 34, 6, 0u) DWBC_ROW_GC(39, 34, 12, lp::kWideTasks)
    DWBC_ROW_REDIST(39, 34, TopoTocabi, 1) DWBC_ROW_REDIST(39, 34, TopoGeneric, 0)
    DWBC_ROW_GRAVCOMP(39, 34, TopoTocabi, 1) DWBC_ROW_GRAVCOMP(39, 34, TopoGeneric, 0)
    DWBC_ROW_LINK_QUERY(39, 34)
    DWBC_ROW_DYNAMICS(39, 34, TopoTocabi, 1) DWBC_ROW_DYNAMICS(39, 34, TopoGeneric, 0)
    DWBC_ROW_CONTACT_SPACE(39, 34, TopoTocabi, 1) DWBC_ROW_CONTACT_SPACE(39, 34, TopoGeneric, 0)
};
#endif
// (the built-in task-space and task-QP rows are emitted by translation units of their own, dwbc_kernels_task_space.hip and
// dwbc_kernels_task_qp.hip: the code objects of the kernels above stay the ones they were whatever those kernels grow into)

// what a pack and the library that loads it must agree on (both are built from this header): the sizes of the shared structures
// and a hash of the kernel sources (Makefile: DWBC_SRC_HASH), so that a pack left over from older kernel code is refused
#ifndef DWBC_SRC_HASH
#define DWBC_SRC_HASH 0u
#endif
inline unsigned kernel_abi_tag() { return (unsigned)(DWBC_SRC_HASH) ^ (unsigned)(sizeof(Setup) * 2654435761u) ^ (unsigned)(sizeof(BatchIO) * 40503u) ^ (unsigned)(DG_COUNT * 97u) ^ (unsigned)sizeof(lp::Row); }

}  // namespace dwbc
