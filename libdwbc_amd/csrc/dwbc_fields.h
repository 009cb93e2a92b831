// dwbc_fields.h -- the data fields of the C-ABI (enum dwbc_field, include/dwbc_batch.h): one row per field with its name, element type,
// per-instance shape and where it lives.  Host only, no HIP header: dwbc_capi.hip derives dwbc_batch_field_bytes / get / bind_device /
// host_ptr and dwbc_field_describe from the rows, the Python layer and the facade read them through those entry points, and
// tests/test_field_table.py pins them.  A new field is one enumerator and one row.
#pragma once
#include <cstddef>

#include "../../include/dwbc_batch.h"
#include "dwbc_types.h"

namespace dwbc_fields {
using namespace dwbc;

// device buffers of a batch that are owned or bound, sized once and uploaded from a host mirror if they have one: the bindable fields,
// the diagnostics record, and the inputs that are no field -- the task-reference inputs and the per-instance parameter record
// and the four outputs of a link query, the three of a gravity compensation the seven of a dynamics launch and the eleven of a contact-space launch, which are no field either (dwbc_batch::buf is indexed by this)
enum Slot { kQ, kFlags, kFstar, kTauIn, kTau, kWrench, kStatus, kRdTau, kRdCf, kRdWrench, kRdStatus, kDiag, kQdot, kTraj, kCtime, kCustom, kInstPar,
            kLqPos, kLqRot, kLqVel, kLqJac, kGvTau, kGvWrench, kGvStatus, kDyA, kDyAInv, kDyB, kDyG, kDyCmm, kDyCom, kDyStatus,
            kCoJC, kCoLambda, kCoJCInvT, kCoNC, kCoAInvNC, kCoW, kCoWInv, kCoNwJw, kCoPos, kCoRot, kCoStatus, kSlotCount };
static_assert(kCoLambda == kCoJC + DWBC_CS_LAMBDA_C && kCoJCInvT == kCoJC + DWBC_CS_J_C_INV_T && kCoNC == kCoJC + DWBC_CS_N_C && kCoAInvNC == kCoJC + DWBC_CS_A_INV_N_C &&
                  kCoW == kCoJC + DWBC_CS_W && kCoWInv == kCoJC + DWBC_CS_W_INV && kCoNwJw == kCoJC + DWBC_CS_NWJW && kCoPos == kCoJC + DWBC_CS_CONTACT_POS &&
                  kCoRot == kCoJC + DWBC_CS_CONTACT_ROT && kCoStatus == kCoJC + DWBC_CS_STATUS, "kCoJC + dwbc_contact_space_output");
static_assert(kDyAInv == kDyA + DWBC_DYN_A_INV && kDyB == kDyA + DWBC_DYN_B && kDyG == kDyA + DWBC_DYN_G && kDyCmm == kDyA + DWBC_DYN_CMM &&
                  kDyCom == kDyA + DWBC_DYN_COM && kDyStatus == kDyA + DWBC_DYN_STATUS, "kDyA + dwbc_dynamics_output");
static_assert(kGvWrench == kGvTau + DWBC_GRAV_WRENCH && kGvStatus == kGvTau + DWBC_GRAV_STATUS, "kGvTau + dwbc_grav_output");
static_assert(kLqRot == kLqPos + DWBC_LQ_ROT && kLqVel == kLqPos + DWBC_LQ_VEL && kLqJac == kLqPos + DWBC_LQ_JAC, "kLqPos + dwbc_link_query_output");

// one extent of a shape: mul * var + add
enum Var { kOne, kN, kM, kNc, kContacts, kFstarTotal, kActive, kDumpTotal };
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
inline int extent(const Dim &d, const dwbc_field_dims &s) {
    const int v[] = {1, s.n, s.n - 6, s.n - 12, s.n_contacts, s.fstar_total, s.max_active, d.var == kDumpTotal ? DumpLayout::make(s.n).total : 0};
    return d.mul * v[d.var] + d.add;
}
inline size_t elements(const Row &r, const dwbc_field_dims &s) {  // per instance
    size_t n = 1;
    for (int i = 0; i < r.shape.rank; i++) n *= (size_t)extent(r.shape.dim[i], s);
    return n;
}
inline size_t item_size(int type) { return type == DWBC_ELEM_F64 ? sizeof(double) : type == DWBC_ELEM_I32 ? sizeof(int) : 1; }

}  // namespace dwbc_fields
