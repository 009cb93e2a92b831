// dwbc_fields.h -- the data fields of the C-ABI (enum dwbc_field, include/dwbc_batch.h): one row per field with its name, element type,
// per-instance shape and where it lives.  Host only, no HIP header: dwbc_capi.hip derives dwbc_batch_field_bytes / get / bind_device /
// host_ptr and dwbc_field_describe from the rows, the Python layer and the facade read them through those entry points, and
// tests/test_field_table.py pins them.  A new field is one enumerator and one row.  A second table, at the end, does the same for the
// outputs of the lean launches, a third and a fourth for those of the task-space and the single-level task-QP launch.
#pragma once
#include <cstddef>

#include "../../include/dwbc_batch.h"
#include "dwbc_types.h"

namespace dwbc_fields {
using namespace dwbc;

// device buffers of a batch that are owned or bound, sized once and uploaded from a host mirror if they have one: the bindable fields,
// the diagnostics record, the inputs that are no field (the task-reference inputs and the per-instance parameter record), and the outputs of
// the lean launches, which are no field either: the table at the end of this file describes them (dwbc_batch::buf is indexed by this)
enum Slot { kQ, kFlags, kFstar, kTauIn, kTau, kWrench, kStatus, kRdTau, kRdCf, kRdWrench, kRdStatus, kDiag, kQdot, kTraj, kCtime, kCustom, kInstPar,
            kLqPos, kLqRot, kLqVel, kLqJac, kGvTau, kGvWrench, kGvStatus, kDyA, kDyAInv, kDyB, kDyG, kDyCmm, kDyCom, kDyStatus,
            kCoJC, kCoLambda, kCoJCInvT, kCoNC, kCoAInvNC, kCoW, kCoWInv, kCoNwJw, kCoPos, kCoRot, kCoStatus,
            // the task-space launch: output `what` of level l in slot kTsFirst + what * kMaxLevels + l, then the one status
            kTsFirst, kTsStatusSlot = kTsFirst + 4 * kMaxLevels,
            kInstModel,  // the per-instance body tables (dwbc_batch_set_instance_model): an input that is no field, like kInstPar
            // the single-level task-QP launch: its two inputs (no field either), then its outputs in the order of enum dwbc_task_qp_output
            kTqTorquePrev, kTqNull, kTqFstarQp, kTqContactQp, kTqTorqueH, kTqTorqueNullH, kTqTorqueContact, kTqStatus,
            kSlotCount };

// one extent of a shape: mul * var + add
enum Var { kOne, kN, kM, kNc, kContacts, kFstarTotal, kActive, kDumpTotal, kQueried, kTaskDof };
struct Dim {
    int mul, var, add;
};
struct Shape {
    int rank;
    Dim dim[3];
};
constexpr Dim c(int k) { return {k, kOne, 0}; }
constexpr Dim N{1, kN, 0}, M{1, kM, 0}, Nc{1, kNc, 0};  // system dof, joints (n - 6), joints off the contact chains (n - 12)
constexpr Shape sh() { return {0, {}}; }
constexpr Shape sh(Dim a) { return {1, {a}}; }
constexpr Shape sh(Dim a, Dim b) { return {2, {a, b}}; }
constexpr Shape sh(Dim a, Dim b, Dim d) { return {3, {a, b, d}}; }

enum Where { kInSlot, kInDump, kTauPart };  // a buffer slot; the dump record; a selection of DWBC_TAU formed by dwbc_tau_select
enum : unsigned { kBindable = 1, kMirror = 2 };

struct Row {
    int id;
    const char *name;  // as libdwbc_amd.Batch.get spells it
    int type;          // DWBC_ELEM_*
    Shape shape;       // per instance, as Batch.get returns it
    int where;
    int idx;                 // kInSlot: the Slot; kTauPart: sel of dwbc_tau_select
    int DumpLayout::*off;    // kInDump: offset inside the record (nullptr: the whole record)
    unsigned flags;
    const char *absent;      // kInSlot: what dwbc_batch_get answers while the buffer does not exist (nullptr: the copy itself fails)
};
constexpr Row slot(int id, const char *name, int type, Shape s, int sl, unsigned flags = 0, const char *absent = nullptr) {
    return {id, name, type, s, kInSlot, sl, nullptr, flags, absent};
}
constexpr Row dump(int id, const char *name, Shape s, int DumpLayout::*off) { return {id, name, DWBC_ELEM_F64, s, kInDump, 0, off, 0, nullptr}; }
constexpr Row tau(int id, const char *name, int sel) { return {id, name, DWBC_ELEM_F64, sh(M), kTauPart, sel, nullptr, 0, nullptr}; }

constexpr int C = 6 * kMaxActiveContacts, K = C - 6, T = kMaxTaskDof, L = kMaxLevels, R = kMaxReducedDof;
constexpr const char *kNoRedist = "no redistribution output yet: call dwbc_batch_redistribute first";
using DL = DumpLayout;

inline constexpr Row kRows[] = {
    slot(DWBC_IN_Q, "in_q", DWBC_ELEM_F64, sh({1, kN, 1}), kQ, kBindable | kMirror),
    slot(DWBC_IN_CONTACT, "in_contact", DWBC_ELEM_U8, sh({1, kContacts, 0}), kFlags, kBindable | kMirror),
    slot(DWBC_IN_FSTAR, "in_fstar", DWBC_ELEM_F64, sh({1, kFstarTotal, 0}), kFstar, kBindable | kMirror),
    slot(DWBC_IN_TORQUE, "in_torque", DWBC_ELEM_F64, sh(M), kTauIn, kBindable | kMirror, "no torque input on the device yet"),
    slot(DWBC_TAU, "tau", DWBC_ELEM_F64, sh(c(3), M), kTau, kBindable),
    slot(DWBC_WRENCH, "wrench", DWBC_ELEM_F64, sh({6, kActive, 0}), kWrench, kBindable),
    slot(DWBC_STATUS, "status", DWBC_ELEM_I32, sh(), kStatus, kBindable),
    slot(DWBC_DIAG, "diag", DWBC_ELEM_I32, sh(c(DG_COUNT)), kDiag),
    slot(DWBC_REDIST_TAU, "redist_tau", DWBC_ELEM_F64, sh(M), kRdTau, kBindable, kNoRedist),
    slot(DWBC_REDIST_CF, "redist_cf", DWBC_ELEM_F64, sh(c(K)), kRdCf, kBindable, kNoRedist),
    slot(DWBC_REDIST_WRENCH, "redist_wrench", DWBC_ELEM_F64, sh(c(2), c(C)), kRdWrench, kBindable, kNoRedist),
    slot(DWBC_REDIST_STATUS, "redist_status", DWBC_ELEM_I32, sh(), kRdStatus, kBindable, kNoRedist),
    tau(DWBC_TAU_GRAV, "tau_grav", 0),
    tau(DWBC_TAU_TASK, "tau_task", 1),
    tau(DWBC_TAU_CONTACT, "tau_contact", 2),
    tau(DWBC_TAU_TOTAL, "tau_total", 3),
    dump(DWBC_A, "A", sh(N, N), &DL::A),
    dump(DWBC_A_INV, "A_inv", sh(N, N), &DL::A_inv),
    dump(DWBC_J_C, "J_C", sh(c(C), N), &DL::J_C),
    dump(DWBC_LAMBDA_C, "Lambda_c", sh(c(C * C)), &DL::Lambda_c),
    dump(DWBC_J_C_INV_T, "J_C_INV_T", sh(c(C), N), &DL::J_C_INV_T),
    dump(DWBC_A_INV_N_C, "A_inv_N_C", sh(N, N), &DL::A_inv_N_C),
    dump(DWBC_W_INV, "W_inv", sh(M, M), &DL::W_inv),
    dump(DWBC_NWJW, "NwJw", sh(M, c(K)), &DL::NwJw),
    dump(DWBC_G, "G", sh(N), &DL::G),
    dump(DWBC_P_C, "P_C", sh(c(C)), &DL::P_C),
    dump(DWBC_LINK_R, "link_R", sh(c(kMaxBodies), c(3), c(3)), &DL::link_R),
    dump(DWBC_LINK_P, "link_p", sh(c(kMaxBodies), c(3)), &DL::link_p),
    dump(DWBC_FSTAR_QP, "fstar_qp", sh(c(L), c(T)), &DL::fstar_qp),
    dump(DWBC_CONTACT_QP, "contact_qp", sh(c(L), c(K)), &DL::contact_qp),
    dump(DWBC_CF_REDIS, "cf_redis", sh(c(K)), &DL::cf_redis),
    dump(DWBC_J_TASK, "J_task", sh(c(L), {T, kN, 0}), &DL::J_task),
    dump(DWBC_LAMBDA_TASK, "Lambda_task", sh(c(L), c(T * T)), &DL::Lambda_task),
    dump(DWBC_J_KT, "J_kt", sh(c(L), {T, kM, 0}), &DL::J_kt),
    dump(DWBC_QP_VIOL, "qp_viol", sh(c(L + 1)), &DL::qp_viol),
    dump(DWBC_DUMP_RAW, "dump_raw", sh({1, kDumpTotal, 0}), nullptr),
    dump(DWBC_CMM, "CMM", sh(c(6), N), &DL::CMM),
    dump(DWBC_COM, "com", sh(c(3)), &DL::com),
    dump(DWBC_COM_INERTIA, "com_inertia", sh(c(3), c(3)), &DL::com_inertia),
    dump(DWBC_J_COM, "J_com", sh(c(6), N), &DL::J_com),
    dump(DWBC_B, "B", sh(N), &DL::B),
    dump(DWBC_LINK_V, "link_v", sh(c(kMaxBodies), c(3)), &DL::link_v),
    dump(DWBC_LINK_W, "link_w", sh(c(kMaxBodies), c(3)), &DL::link_w),
    dump(DWBC_CONTACT_POS, "contact_pos", sh(c(kMaxActiveContacts), c(3)), &DL::contact_pos),
    dump(DWBC_CONTACT_ROT, "contact_rot", sh(c(kMaxActiveContacts), c(3), c(3)), &DL::contact_rot),
    dump(DWBC_ZMP, "zmp", sh(c(1 + kMaxActiveContacts), c(3)), &DL::zmp),
    dump(DWBC_A_R, "A_R", sh(c(R), c(R)), &DL::A_R),
    dump(DWBC_A_R_INV, "A_R_inv", sh(c(R), c(R)), &DL::A_R_inv),
    dump(DWBC_G_R, "G_R", sh(c(R)), &DL::G_R),
    dump(DWBC_J_I_NC, "J_I_nc", sh(c(6), Nc), &DL::J_I_nc),
    dump(DWBC_J_I_NC_INV_T, "J_I_nc_inv_T", sh(c(6), Nc), &DL::J_I_nc_inv_T),
};
constexpr int kRowCount = (int)(sizeof(kRows) / sizeof(kRows[0]));

inline const Row *find(int id) {
    for (const Row &r : kRows)
        if (r.id == id) return &r;
    return nullptr;
}
// n_queried: entries of the link query; t: task dof of the level a task-space output belongs to (dwbc_field_dims is ABI and has no place
// for either; no field depends on them)
inline int extent(const Dim &d, const dwbc_field_dims &s, int n_queried = 0, int t = 0) {
    const int v[] = {1, s.n, s.n - 6, s.n - 12, s.n_contacts, s.fstar_total, s.max_active, d.var == kDumpTotal ? DumpLayout::make(s.n).total : 0, n_queried, t};
    return d.mul * v[d.var] + d.add;
}
inline size_t elements(const Shape &shape, const dwbc_field_dims &s, int n_queried = 0, int t = 0) {  // per instance
    size_t n = 1;
    for (int i = 0; i < shape.rank; i++) n *= (size_t)extent(shape.dim[i], s, n_queried, t);
    return n;
}
inline size_t item_size(int type) { return type == DWBC_ELEM_F64 ? sizeof(double) : type == DWBC_ELEM_I32 ? sizeof(int) : 1; }
// what dwbc_field_describe and dwbc_lean_output_describe answer for a row of either table
inline dwbc_field_info describe(int id, const char *name, int type, const Shape &shape, const dwbc_field_dims &s, int n_queried, bool bindable, bool mirror,
                                int t = 0) {
    dwbc_field_info o{id, name, type, shape.rank, {1, 1, 1}, elements(shape, s, n_queried, t) * item_size(type), bindable, mirror};
    for (int i = 0; i < shape.rank; i++) o.dims[i] = extent(shape.dim[i], s, n_queried, t);
    return o;
}

// ---- the outputs of the lean launches (enum dwbc_lean_family): per family one block with a row per output of its enum, in enumerator
// order, and the messages of its refusals.  Output i of a family lives in slot rows[0].slot + i, is part of a request when bit i of the
// family's mask (dwbc_batch::lean) is set, and is sized by its shape: dwbc_capi.hip derives *_bytes / get_* / bind_* and the allocation
// of a request from the rows, the Python layer reads them through dwbc_lean_output_describe, and tests/test_lean_output_table.py pins them.
// A new lean launch is one block here and one launch function there.
struct LeanRow {
    int id, slot;  // the output's enumerator and its Slot
    const char *name;  // as libdwbc_amd.Batch spells it
    int type;
    Shape shape;  // per instance
};
struct Family {
    const LeanRow *rows;
    int count;
    int status;  // index of the status output, which every request implies (-1: none)
    // refusals (nullptr: the family has no such case): no such output; an unknown bit in a request; nothing requested; the output is not
    // part of the request; no launch has filled the outputs yet
    const char *unknown, *unknown_bit, *no_request, *not_asked, *not_run;
    constexpr unsigned all() const { return (1u << count) - 1u; }
};
template <int N>
constexpr Family family(const LeanRow (&rows)[N], int status, const char *unknown, const char *unknown_bit, const char *no_request, const char *not_asked, const char *not_run) {
    return {rows, N, status, unknown, unknown_bit, no_request, not_asked, not_run};
}
constexpr Dim Q{1, kQueried, 0};  // entries of the link query
constexpr int F64 = DWBC_ELEM_F64, I32 = DWBC_ELEM_I32;

inline constexpr LeanRow kGravRows[] = {
    {DWBC_GRAV_TAU, kGvTau, "tau", F64, sh(M)},
    {DWBC_GRAV_WRENCH, kGvWrench, "wrench", F64, sh(c(12))},
    {DWBC_GRAV_STATUS, kGvStatus, "status", I32, sh()},
};
inline constexpr LeanRow kLinkQueryRows[] = {
    {DWBC_LQ_POS, kLqPos, "pos", F64, sh(Q, c(3))},
    {DWBC_LQ_ROT, kLqRot, "rot", F64, sh(Q, c(3), c(3))},
    {DWBC_LQ_VEL, kLqVel, "vel", F64, sh(Q, c(6))},
    {DWBC_LQ_JAC, kLqJac, "jac", F64, sh(Q, c(6), N)},  // part of the request only when the query asks for Jacobians
};
inline constexpr LeanRow kDynamicsRows[] = {
    {DWBC_DYN_A, kDyA, "A", F64, sh(N, N)},
    {DWBC_DYN_A_INV, kDyAInv, "A_inv", F64, sh(N, N)},
    {DWBC_DYN_B, kDyB, "B", F64, sh(N)},
    {DWBC_DYN_G, kDyG, "G", F64, sh(N)},
    {DWBC_DYN_CMM, kDyCmm, "CMM", F64, sh(c(6), N)},
    {DWBC_DYN_COM, kDyCom, "com", F64, sh(c(3))},
    {DWBC_DYN_STATUS, kDyStatus, "status", I32, sh()},
};
inline constexpr LeanRow kContactSpaceRows[] = {
    {DWBC_CS_J_C, kCoJC, "J_C", F64, sh(c(12), N)},
    {DWBC_CS_LAMBDA_C, kCoLambda, "Lambda_c", F64, sh(c(12), c(12))},
    {DWBC_CS_J_C_INV_T, kCoJCInvT, "J_C_INV_T", F64, sh(c(12), N)},
    {DWBC_CS_N_C, kCoNC, "N_C", F64, sh(N, N)},
    {DWBC_CS_A_INV_N_C, kCoAInvNC, "A_inv_N_C", F64, sh(N, N)},
    {DWBC_CS_W, kCoW, "W", F64, sh(M, M)},
    {DWBC_CS_W_INV, kCoWInv, "W_inv", F64, sh(M, M)},
    {DWBC_CS_NWJW, kCoNwJw, "NwJw", F64, sh(M, c(6))},
    {DWBC_CS_CONTACT_POS, kCoPos, "contact_pos", F64, sh(c(2), c(3))},
    {DWBC_CS_CONTACT_ROT, kCoRot, "contact_rot", F64, sh(c(2), c(3), c(3))},
    {DWBC_CS_STATUS, kCoStatus, "status", I32, sh()},
};
// indexed by enum dwbc_lean_family
inline constexpr Family kLean[] = {
    family(kGravRows, DWBC_GRAV_STATUS, "gravity compensation: unknown output", nullptr, nullptr, nullptr,
           "no gravity-compensation output yet: call dwbc_batch_grav_compensation (or dwbc_batch_redistribute with DWBC_REDIST_ADD_GRAVITY) first"),
    family(kLinkQueryRows, -1, "link query: unknown output", nullptr, "no link query: call dwbc_batch_set_link_query first",
           "link query: set without Jacobians (dwbc_batch_set_link_query with want_jacobians = 1)", "no link-query output yet: call dwbc_batch_update_kinematics first"),
    family(kDynamicsRows, DWBC_DYN_STATUS, "dynamics: unknown output", "dynamics: unknown output bit (the outputs are 1u << DWBC_DYN_A .. 1u << DWBC_DYN_STATUS)",
           "no dynamics request: call dwbc_batch_set_dynamics_outputs first", "dynamics: this output was not asked for (dwbc_batch_set_dynamics_outputs)",
           "no dynamics output yet: call dwbc_batch_update_dynamics first"),
    family(kContactSpaceRows, DWBC_CS_STATUS, "contact space: unknown output",
           "contact space: unknown output bit (the outputs are 1u << DWBC_CS_J_C .. 1u << DWBC_CS_STATUS)",
           "no contact-space request: call dwbc_batch_set_contact_space_outputs first",
           "contact space: this output was not asked for (dwbc_batch_set_contact_space_outputs)",
           "no contact-space output yet: call dwbc_batch_calc_contact_constraint first"),
};
constexpr int kLeanCount = (int)(sizeof(kLean) / sizeof(kLean[0]));
constexpr bool lean_rows_in_order() {
    for (const Family &f : kLean)
        for (int i = 0; i < f.count; i++)
            if (f.rows[i].id != i || f.rows[i].slot != f.rows[0].slot + i) return false;
    return true;
}
static_assert(lean_rows_in_order(), "row i of a lean family is enumerator i of its output enum and lives in slot rows[0].slot + i");
static_assert(kLean[DWBC_LEAN_GRAV].rows == kGravRows && kLean[DWBC_LEAN_LINK_QUERY].rows == kLinkQueryRows && kLean[DWBC_LEAN_DYNAMICS].rows == kDynamicsRows &&
                  kLean[DWBC_LEAN_CONTACT_SPACE].rows == kContactSpaceRows && kLeanCount == 4,"kLean is indexed by dwbc_lean_family");

// ---- the outputs of the task-space launch (enum dwbc_task_space_output): no family of kLean -- every output but the status exists once per
// task level, in the shape of that level's task dof.  Row i is enumerator i; output i of level l lives in slot kTsFirst + i * kMaxLevels + l
// (the status in kTsStatusSlot) and is part of a request when bit i of dwbc_batch::ts.mask is set.  dwbc_capi.hip derives
// dwbc_batch_task_space_bytes / get / bind and the allocation of a request from the rows, the Python layer reads them through
// dwbc_task_space_output_describe.
constexpr Dim Tt{1, kTaskDof, 0};  // task dof of the level
inline constexpr LeanRow kTaskSpaceRows[] = {
    {DWBC_TS_J_TASK, kTsFirst, "J_task", F64, sh(Tt, N)},
    {DWBC_TS_LAMBDA_TASK, kTsFirst + kMaxLevels, "Lambda_task", F64, sh(Tt, Tt)},
    {DWBC_TS_J_KT, kTsFirst + 2 * kMaxLevels, "J_kt", F64, sh(M, Tt)},
    {DWBC_TS_NULL_TASK, kTsFirst + 3 * kMaxLevels, "Null_task", F64, sh(M, M)},
    {DWBC_TS_STATUS, kTsStatusSlot, "status", I32, sh()},
};
inline constexpr Family kTaskSpace =
    family(kTaskSpaceRows, DWBC_TS_STATUS, "task space: unknown output", "task space: unknown output bit (the outputs are 1u << DWBC_TS_J_TASK .. 1u << DWBC_TS_STATUS)",
           "no task-space request: call dwbc_batch_set_task_space_outputs first", "task space: this output was not asked for (dwbc_batch_set_task_space_outputs)",
           "no task-space output yet: call dwbc_batch_calc_task_space first");
constexpr bool task_space_rows_in_order() {
    for (int i = 0; i < kTaskSpace.count; i++)
        if (kTaskSpaceRows[i].id != i || kTaskSpaceRows[i].slot != (i == DWBC_TS_STATUS ? (int)kTsStatusSlot : kTsFirst + i * kMaxLevels)) return false;
    return true;
}
static_assert(task_space_rows_in_order() && kTaskSpace.count == DWBC_TS_STATUS + 1, "row i of the task-space table is enumerator i of dwbc_task_space_output");

// ---- the outputs of the single-level task-QP launch (enum dwbc_task_qp_output): a table of its own, no family of kLean (that table is
// the four launches that read the state alone; this one has inputs and a level of its own: dwbc_batch::tq).  Row i is enumerator i and lives
// in slot kTqFstarQp + i; dwbc_capi.hip derives dwbc_batch_task_qp_bytes / get / bind and the allocation of a request from the rows, the
// Python layer reads them through dwbc_task_qp_output_describe.
inline constexpr LeanRow kTaskQpRows[] = {
    {DWBC_TQ_F_STAR_QP, kTqFstarQp, "f_star_qp", F64, sh(c(T))},
    {DWBC_TQ_CONTACT_QP, kTqContactQp, "contact_qp", F64, sh(c(K))},
    {DWBC_TQ_TORQUE_H, kTqTorqueH, "torque_h", F64, sh(M)},
    {DWBC_TQ_TORQUE_NULL_H, kTqTorqueNullH, "torque_null_h", F64, sh(M)},
    {DWBC_TQ_TORQUE_CONTACT, kTqTorqueContact, "torque_contact", F64, sh(M)},
    {DWBC_TQ_STATUS, kTqStatus, "status", I32, sh()},
};
inline constexpr Family kTaskQp =
    family(kTaskQpRows, DWBC_TQ_STATUS, "single-level task QP: unknown output",
           "single-level task QP: unknown output bit (the outputs are 1u << DWBC_TQ_F_STAR_QP .. 1u << DWBC_TQ_STATUS)",
           "no single-level task-QP request: call dwbc_batch_set_task_qp first", "single-level task QP: this output was not asked for (dwbc_batch_set_task_qp)",
           "no single-level task-QP output yet: call dwbc_batch_calc_single_task_torque_qp first");
constexpr bool task_qp_rows_in_order() {
    for (int i = 0; i < kTaskQp.count; i++)
        if (kTaskQpRows[i].id != i || kTaskQpRows[i].slot != kTqFstarQp + i) return false;
    return true;
}
static_assert(task_qp_rows_in_order() && kTaskQp.count == DWBC_TQ_STATUS + 1, "row i of the task-QP table is enumerator i of dwbc_task_qp_output");

}  // namespace dwbc_fields
