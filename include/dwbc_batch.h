/*
 * dwbc_batch.h -- C-ABI of the MI355X-native batched libdwbc hot path (libdwbc_hip.so).
 *
 * The reference (saga0619/libdwbc) has no FFI: its boundary is the C++ class DWBC::RobotData
 * (reference include/dwbc.h:59-430).  Each entry point below replaces the RobotData method cited next to
 * it, for B independent robot instances at once; include/dwbc_amd.hpp is the header-only C++ facade that
 * gives the RobotData names/arguments back on top of this ABI (B = 1 reproduces single-robot behaviour).
 *
 * Conventions (same as the reference): q = [x y z | qx qy qz | joints | qw] (size ndof+1), qdot/qddot size
 * ndof with the base angular velocity in the body frame; Jacobian rows / wrenches are [linear; angular] in
 * the world frame; int returns are 1 = ok, 0 = failure (no exceptions); failures leave a message in
 * dwbc_last_error().  Host arrays are instance-major (AoS), double precision.
 * Not thread-safe per object (one dwbc_batch per thread), like RobotData.
 */
#ifndef DWBC_BATCH_H
#define DWBC_BATCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dwbc_model dwbc_model;
typedef struct dwbc_batch dwbc_batch;

/* contact types: reference include/dwbc_contact_constraint.h:19-25 */
enum { DWBC_CONTACT_6D = 0, DWBC_CONTACT_POINT = 1, DWBC_CONTACT_LINK = 2, DWBC_CONTACT_LINE = 3 };
/* task link modes: reference include/dwbc_task.h:23-33 */
enum {
    DWBC_TASK_LINK_6D = 0, DWBC_TASK_LINK_6D_COM_FRAME, DWBC_TASK_LINK_6D_CUSTOM_FRAME,
    DWBC_TASK_LINK_POSITION, DWBC_TASK_LINK_POSITION_COM_FRAME, DWBC_TASK_LINK_POSITION_CUSTOM_FRAME,
    DWBC_TASK_LINK_ROTATION, DWBC_TASK_LINK_ROTATION_CUSTOM_FRAME
};
/* arithmetic type of the kernels.  DWBC_F32 runs the same kernel source in single precision; every buffer at this boundary
 * (host arrays, bound device buffers) stays double and is converted inside the kernel.  Accuracy envelope: DESIGN.md §8 */
enum { DWBC_F64 = 0, DWBC_F32 = 1 };
/* DWBC_SOLVE_HQP: CalcTaskControlTorque(hqp) / CalcContactRedistribute(hqp) with hqp = true (the QP cascade); without the bit the
 * plain hierarchy and the closed-form two-contact redistribution run (src/dwbc.cpp:856-873, 1570-1619), full model only.
 * DWBC_SOLVE_REDUCED: the Reduced* call sequence (ReducedDynamicsCalculate, ReducedCalcContactConstraint,
 * ReducedCalcGravCompensation, ReducedCalcTaskSpace, ReducedCalcTaskControlTorque, ReducedCalcContactRedistribute --
 * reference include/dwbc.h:411-416, tests/sp_test/redu_dyn_test.cpp:263-298) instead of the full-model sequence.
 * DWBC_SOLVE_INIT: the `init` argument of CalcTaskControlTorque / CalcContactRedistribute.  Set: cold start (qpOASES init).
 * Clear: hot start (qpOASES hotstart, src/qp_wrapper.cpp:249-296) -- every QP of the full-model path first visits the rows of
 * its working set from the previous dwbc_batch_solve on this batch (kept in HBM); the returned point is the same canonical
 * point, only the number of active-set steps changes.  The first solve of a batch always runs cold.  The failure fallback of
 * SolveQPoases (fresh problem, setToReliable, nWSR x 10, src/qp_wrapper.cpp:298-339) has no counterpart to switch to: the
 * device solver has no heuristic options, its step budget is the reference's nWSR + 10 nWSR. */
enum { DWBC_SOLVE_HQP = 1, DWBC_SOLVE_INIT = 2, DWBC_SOLVE_REDUCED = 4 };

/* fields for dwbc_batch_get / dwbc_batch_bind_device.  Shapes are per instance, row-major. */
enum dwbc_field {
    /* inputs (bindable) */
    DWBC_IN_Q = 0,        /* (ndof+1)        f64  -- UpdateKinematics(q, ...)          */
    DWBC_IN_CONTACT = 1,  /* (n_contacts)    u8   -- SetContact(...)                   */
    DWBC_IN_FSTAR = 2,    /* (sum task dof)  f64  -- SetTaskSpace(level, f*) concatenated */
    DWBC_IN_TORQUE = 3,   /* (m)             f64  -- torque_input of CalcContactRedistribute(torque_input, ...) (dwbc_batch_redistribute) */
    /* outputs (bindable) */
    DWBC_TAU = 10,        /* (3, m) f64: torque_grav_, torque_task_, torque_contact_  (include/dwbc.h:115-117) */
    DWBC_WRENCH = 11,     /* (12; 18 after dwbc_batch_set_max_active_contacts(b, 3)) f64: getContactForce(tau_total), zero padded (src/dwbc.cpp:891-896) */
    DWBC_STATUS = 12,     /* (1)    i32: 1 ok / 0 failed                               */
    DWBC_DIAG = 13,       /* (90)   i32: stage status, QP iterations, working sets, stage stamps */
    /* outputs of dwbc_batch_redistribute (bindable) */
    DWBC_REDIST_TAU = 14,    /* (m)     f64: NwJw c, what CalcContactRedistribute(torque_input) adds to torque_contact_ (src/dwbc.cpp:1549) */
    DWBC_REDIST_CF = 15,     /* (6)     f64: c = cf_redis_qp_, zero beyond the contact-null dimension */
    DWBC_REDIST_WRENCH = 16, /* (2, 12) f64: getContactForce(torque_input), getContactForce(torque_input + NwJw c); zero padded */
    DWBC_REDIST_STATUS = 17, /* (1)     i32: 1 ok / 0 failed */
    /* derived getters (host only) */
    DWBC_TAU_GRAV = 20, DWBC_TAU_TASK = 21, DWBC_TAU_CONTACT = 22, DWBC_TAU_TOTAL = 23,
    /* intermediates, available after a solve with dwbc_batch_enable_dump(b, 1) -- the RobotData public fields */
    DWBC_A = 30,          /* (n, n)   A_        */
    DWBC_A_INV = 31,      /* (n, n)   A_inv_    */
    DWBC_J_C = 32,        /* (12, n)  J_C       */
    DWBC_LAMBDA_C = 33,   /* (12, 12) Lambda_contact (row stride = active contact dof) */
    DWBC_J_C_INV_T = 34,  /* (12, n)  J_C_INV_T */
    DWBC_A_INV_N_C = 35,  /* (n, n)   A_inv_N_C */
    DWBC_W_INV = 36,      /* (m, m)   W_inv     */
    DWBC_NWJW = 37,       /* (m, 6)   NwJw      */
    DWBC_G = 38,          /* (n)      G_        */
    DWBC_P_C = 39,        /* (12)     P_C       */
    DWBC_LINK_R = 40,     /* (48, 9)  link_[i].rotm */
    DWBC_LINK_P = 41,     /* (48, 3)  link_[i].xpos */
    DWBC_FSTAR_QP = 42,   /* (4, 6)   ts_[l].f_star_qp_  */
    DWBC_CONTACT_QP = 43, /* (4, 6)   ts_[l].contact_qp_ */
    DWBC_CF_REDIS = 44,   /* (6)      cf_redis_qp_       */
    DWBC_J_TASK = 45,     /* (4, 6, n) ts_[l].J_task_ (row stride n)       */
    DWBC_LAMBDA_TASK = 46,/* (4, 36)  ts_[l].Lambda_task_ (row stride t_l) */
    DWBC_J_KT = 47,       /* (4, m*6) ts_[l].J_kt_ (row stride t_l)        */
    DWBC_QP_VIOL = 48,    /* (5)      worst normalised slack of each QP's returned point */
    DWBC_DUMP_RAW = 49,   /* whole dump record */
    DWBC_CMM = 50,        /* (6, n)   CMM_                      (src/dwbc.cpp:336) */
    DWBC_COM = 51,        /* (3)      com_pos                   (src/dwbc.cpp:322) */
    DWBC_COM_INERTIA = 52,/* (3, 3)   link_.back().inertia      (src/dwbc.cpp:343) */
    DWBC_J_COM = 53,      /* (6, n)   link_.back().jac_com_     (src/dwbc.cpp:352) */
    /* velocity-dependent outputs of UpdateKinematics: need a qdot in dwbc_batch_set_state */
    DWBC_B = 54,          /* (n)      B_ = C qdot + g (RNEA)    (src/dwbc.cpp:343-344) */
    DWBC_LINK_V = 55,     /* (48, 3)  link_[i].v                (src/link.cpp:87) */
    DWBC_LINK_W = 56,     /* (48, 3)  link_[i].w                (src/link.cpp:88) */
    DWBC_CONTACT_POS = 57,/* (2, 3)   cc_[i].xc_pos of the active contacts (src/contact_constraint.cpp:53) */
    DWBC_CONTACT_ROT = 58,/* (2, 9)   cc_[i].rotm */
    DWBC_ZMP = 59,        /* (3, 3)   getZMP(getContactForce(tau_total)) then cc_[i].zmp_pos (src/dwbc.cpp:898-939) */
    /* the reduced (centroidal) model, after a solve with DWBC_SOLVE_REDUCED (src/dwbc.cpp:2932-2988); RS = vc_dof + 6 <= 24 */
    DWBC_A_R = 60,        /* (24, 24) A_R, row stride 24, zero beyond RS */
    DWBC_A_R_INV = 61,    /* (24, 24) A_R_inv */
    DWBC_G_R = 62,        /* (24)     G_R */
    DWBC_J_I_NC = 63,     /* (6, n-12) J_I_nc_, row stride n - 12, zero beyond nc_dof */
    DWBC_J_I_NC_INV_T = 64 /* (6, n-12) J_I_nc_inv_T */
};
/* the table behind the enum, one row per field (libdwbc_amd/csrc/dwbc_fields.h), for a caller that sizes or types its buffers from the
 * library instead of from the comments above: the sizes a shape depends on, and what a row says for them */
enum { DWBC_ELEM_F64 = 0, DWBC_ELEM_I32 = 1, DWBC_ELEM_U8 = 2 };
typedef struct dwbc_field_dims {
    int n;           /* dwbc_model_system_dof */
    int n_contacts;  /* registered contacts */
    int fstar_total; /* dwbc_batch_fstar_size */
    int max_active;  /* dwbc_batch_max_active_contacts */
} dwbc_field_dims;
typedef struct dwbc_field_info {
    int id;           /* enum dwbc_field */
    const char *name; /* as the Python layer spells it: "in_q", "A_inv_N_C", "Lambda_c", ... */
    int dtype;        /* DWBC_ELEM_* */
    int rank;         /* 0 .. 3 */
    int dims[3];      /* per instance, row-major; unused entries are 1 */
    size_t bytes;     /* per instance */
    int bindable;     /* dwbc_batch_bind_device takes it */
    int host_mirror;  /* dwbc_batch_host_ptr serves it */
} dwbc_field_info;
/* row `index` of the field table for the given sizes; 0 when index is past the end.  Needs no device and no batch. */
int dwbc_field_describe(int index, const dwbc_field_dims *dims, dwbc_field_info *out);
/* the lean launches below write outputs that are no dwbc_field: each family has an output enum and get / bind / bytes calls of its own.
 * Their table (libdwbc_amd/csrc/dwbc_fields.h as well) is read like the field table: row `index` of `family` for a model of n dof and a
 * link query of n_queried entries.
 * out->id is the family's output enumerator, bindable 1, host_mirror 0; 0 when index is past the end or there is no such family.  Needs
 * no device and no batch. */
enum dwbc_lean_family { DWBC_LEAN_GRAV = 0, DWBC_LEAN_LINK_QUERY = 1, DWBC_LEAN_DYNAMICS = 2, DWBC_LEAN_CONTACT_SPACE = 3 };
int dwbc_lean_output_describe(int family, int index, int n, int n_queried, dwbc_field_info *out);

const char *dwbc_last_error(void);
int dwbc_device_count(void);

/* ---- model: RobotData::LoadModelData(urdf, floating, verbose)  reference include/dwbc.h:237, src/dwbc.cpp:102-252 */
dwbc_model *dwbc_model_create_from_urdf(const char *urdf_path, int floating_base);
/* same tree given as arrays (R_T: nb x 9 child->parent joint-frame rotation, inertia: nb x 9 about the com) */
dwbc_model *dwbc_model_create_from_arrays(int nb, const int32_t *parent, const double *R_T, const double *p_T,
                                          const double *axis, const double *mass, const double *com,
                                          const double *inertia);
void dwbc_model_destroy(dwbc_model *m);
int dwbc_model_num_links(const dwbc_model *m);   /* link_num_   */
int dwbc_model_system_dof(const dwbc_model *m);  /* system_dof_ */
double dwbc_model_total_mass(const dwbc_model *m); /* total_mass_ */
int dwbc_model_link_id(const dwbc_model *m, const char *name); /* case-insensitive, -1 if absent (src/dwbc.cpp:397-406) */
const char *dwbc_model_link_name(const dwbc_model *m, int link);
int dwbc_model_get_arrays(const dwbc_model *m, int32_t *parent, double *R_T, double *p_T, double *axis, double *mass,
                          double *com, double *inertia);
/* The model as the kernels read it: nb records of 25 doubles, one per body in the order of the arrays above,
 *   [ R_T[9] row-major | p_T[3] | axis[3] | mass | com[3] | Icom xx xy xz yy yz zz ]
 * (joint frame in the parent's frame, joint axis, then the link's mass, COM offset and inertia about the COM in the link frame; body 0 is the
 * floating base, whose axis is not read).  `out` is nb x 25.  This is the record of dwbc_batch_set_instance_model, once per instance. */
int dwbc_model_body_table(const dwbc_model *m, double *out);
/* ---- init-time model surgery (reference include/dwbc.h:206-226, src/dwbc.cpp:1764-2382, 2707-2730).  Each call returns a NEW
 * model (NULL + dwbc_last_error on refusal) and leaves its argument alone: destroy both when done.  A model of another size
 * runs on its own kernel pack (`make -C libdwbc_amd/csrc pack N=.. NB=..`).
 *   DeleteLink(link)                  the link and all its descendants; the links after them move down
 *   AddLink(parent, name, joint_type, axis, joint_rotm, joint_trans, mass, com, inertia)
 *                                     joint_type 0 = JOINT_FIXED: the body is joined to the parent link (RBDL Body::Join), no new link;
 *                                     1 = JOINT_REVOLUTE: a new LAST link whose joint is the last coordinate -- accepted when the parent
 *                                     is the last link or one of its ancestors (the kernels need the depth-first numbering kept)
 *   ChangeLinkToFixedJoint(link)      = DeleteLink(link) + AddLink(fixed) of the link's own body, as the reference does it
 *                                     (src/dwbc.cpp:2360-2382: the link's descendants are deleted with it)
 *   ChangeLinkInertia(link, com_inertia, com_position, com_mass)
 * joint_rotm: 3x3 row-major rotation child -> parent of the joint frame, joint_trans its origin in the parent frame */
dwbc_model *dwbc_model_delete_link(const dwbc_model *m, int link);
dwbc_model *dwbc_model_add_link(const dwbc_model *m, int parent_link, const char *link_name, int joint_type, const double *joint_axis,
                                const double *joint_rotm, const double *joint_trans, double body_mass, const double *com_position,
                                const double *inertia);
dwbc_model *dwbc_model_change_link_to_fixed_joint(const dwbc_model *m, int link);
dwbc_model *dwbc_model_change_link_inertia(const dwbc_model *m, int link, const double *com_inertia, const double *com_position, double com_mass);

/* ---- batch of B RobotData instances sharing one model and one contact/task setup ---- */
dwbc_batch *dwbc_batch_create(const dwbc_model *m, int B, int device, int dtype);
void dwbc_batch_destroy(dwbc_batch *b);
int dwbc_batch_size(const dwbc_batch *b);

/* AddContactConstraint(link, type, point, normal, lx, ly)  include/dwbc.h:259 ; SetFrictionRatio src/contact_constraint.cpp:93.
 * returns the contact index or -1 */
int dwbc_batch_add_contact(dwbc_batch *b, int link, int contact_type, const double point[3], double lx, double ly,
                           double mu, double mu_z);
int dwbc_batch_clear_contacts(dwbc_batch *b);                               /* ClearContactConstraint */
/* AddTaskSpace(level, mode, link, point) include/dwbc.h:319 (same level twice appends a link, src/dwbc.cpp:592-600).
 * link = dwbc_model_num_links(m) (= dwbc_model_link_id(m, "COM")) is the synthetic COM link.  Two 6D links on one level make a
 * 12-dof level: such a batch runs the general-contact kernel (see dwbc_batch_set_max_active_contacts), which takes link and COM
 * levels alike */
int dwbc_batch_add_task(dwbc_batch *b, int level, int mode, int link, const double point[3]);
/* AddTaskSpace(heirarchy, TASK_CUSTOM, task_dof) include/dwbc.h:318 and SetTaskSpace(heirarchy, f*, J_task) include/dwbc.h:333:
 * a level whose Jacobian the caller supplies, per instance (fstar: B x task_dof or NULL to keep, J: B x task_dof x ndof row-major) */
int dwbc_batch_add_custom_task(dwbc_batch *b, int level, int task_dof);
int dwbc_batch_set_custom_task(dwbc_batch *b, int level, const double *fstar, const double *J);
int dwbc_batch_clear_tasks(dwbc_batch *b);                                  /* ClearTaskSpace */
/* ---- on-device task reference (reference src/task.cpp:223-339, src/dwbc.cpp:708-780): a task link with a trajectory gets its
 * f* segment from the quintic / slerp trajectory + PD law on the device; link_index = position of the link inside its level.
 * TaskLink::SetTaskGain(pos_p, pos_d, pos_a, rot_p, rot_d, rot_a)  include/dwbc_task.h:108 (shared by the batch) */
int dwbc_batch_set_task_gain(dwbc_batch *b, int level, int link_index, const double pos_p[3], const double pos_d[3],
                             const double pos_a[3], const double rot_p[3], const double rot_d[3], const double rot_a[3]);
/* TaskLink::SetTrajectoryQuintic + SetTrajectoryRotation  include/dwbc_task.h:104-106 : traj is B x 34 doubles per instance
 *   t_start t_end | pos_init[3] vel_init[3] pos_desired[3] vel_desired[3] | rot_init[9] rot_desired[9] (row-major) |
 *   has_pos has_rot (traj_pos_set / traj_rot_set);  NULL = back to the SetTaskSpace values for this link */
int dwbc_batch_set_trajectory(dwbc_batch *b, int level, int link_index, const double *traj);
/* RobotData::control_time_ (include/dwbc.h:86), one value per instance */
int dwbc_batch_set_control_time(dwbc_batch *b, const double *control_time);
int dwbc_batch_set_torque_limit(dwbc_batch *b, const double *tau_lim);      /* SetTorqueLimit include/dwbc.h:249; NULL = unset */
int dwbc_batch_fstar_size(const dwbc_batch *b);
int dwbc_batch_task_dof(const dwbc_batch *b, int level);
/* Per-instance torque limits and contact cone constants (no counterpart in the reference, where one RobotData is one robot): one record
 * of dwbc_batch_instance_param_stride(b) = m + 4 * n_contacts doubles per instance,
 *   [ tau_lim[0..m) | lx ly mu mu_z of registered contact 0 | ... of contact n_contacts - 1 ]      (registration order, not active order)
 * While a batch has a record, instance i's QP rows -- the task QPs of dwbc_batch_solve and the QP of dwbc_batch_redistribute -- are
 * filled from record i in place of dwbc_batch_set_torque_limit's values and the lx / ly / mu / mu_z of dwbc_batch_add_contact; the
 * torque rows exist exactly as after dwbc_batch_set_torque_limit.  Contact points and links stay per batch.  It is no dwbc_field:
 *   set   host is B x stride; every entry must be finite and > 0, otherwise 0 is returned and the batch keeps what it had.  Uploaded by
 *         the next solve / redistribution on the batch's stream from a page-locked copy.  NULL drops the record: the batch-wide values
 *         hold again.  Refused while a device buffer is bound.
 *   bind  a caller-owned DEVICE buffer of B x stride doubles (a torch tensor), read in place by every later launch: no transfer and no
 *         validation.  NULL unbinds (the batch-wide values hold again).
 * dwbc_batch_add_contact and dwbc_batch_clear_contacts drop the record (the stride changes); dwbc_batch_copy_kinematics does not copy
 * it.  Refused with a record (dwbc_last_error, nothing is launched): DWBC_SOLVE_REDUCED, DWBC_SOLVE_HQP clear (the closed form reads
 * neither limits nor cones), dwbc_batch_configure_lqp* / dwbc_batch_solve_jacc* (one set of contact constants per batch). */
int dwbc_batch_instance_param_stride(const dwbc_batch *b);
int dwbc_batch_set_instance_params(dwbc_batch *b, const double *host);
int dwbc_batch_bind_instance_params(dwbc_batch *b, void *device_ptr);
/* Per-instance link mass, COM, inertia and joint frames (no counterpart in the reference either): one body table per instance,
 * dwbc_batch_instance_model_stride(b) = nb * 25 doubles each, in the layout of dwbc_model_body_table.  While a batch has the record,
 * instance i is computed with table i: the full-model cycle of dwbc_batch_solve on every launch route and the six lean launches
 * (redistribution, gravity compensation, link query, dynamics, contact space, task space) run the dwbc_im:: build of the kernel they would
 * run without it (dwbc_batch_kernel_name says so).  The tree, the contact and task set-up stay per batch; the record and the instance
 * parameters above may be present together.  It is no dwbc_field:
 *   set   host is B x stride.  Checked per body, the reason in dwbc_last_error: every entry finite, mass > 0, inertia diagonal > 0, and for
 *         bodies >= 1 |axis| = 1 and R_T R_T^T = I to 1e-6; on failure 0 is returned and the batch keeps what it had.  Uploaded by the next
 *         launch on the batch's stream from a page-locked copy.  NULL drops the record: the model's own table holds again.  Refused while
 *         a device buffer is bound.
 *   bind  a caller-owned DEVICE buffer of B x stride doubles (a torch tensor), read in place by every later launch: no transfer and no
 *         validation.  NULL unbinds.
 * Both refuse at once: a DWBC_F32 batch, a model that is not on TOCABI's constant tree (another tree of its size, or a batch created under
 * DWBC_DENSE_SWEEP) and a kernel-pack model.  dwbc_batch_copy_kinematics does not copy the record.  Refused with a record (nothing is
 * launched): DWBC_SOLVE_REDUCED, three active contacts or a task level of more than 6 dof (the general-contact kernel),
 * dwbc_batch_configure_lqp* / dwbc_batch_solve_jacc*.  The C++ facade dwbc_amd.hpp does not expose it. */
int dwbc_batch_instance_model_stride(const dwbc_batch *b);
int dwbc_batch_set_instance_model(dwbc_batch *b, const double *host);
int dwbc_batch_bind_instance_model(dwbc_batch *b, void *device_ptr);

/* UpdateKinematics(q, qdot, qddot) include/dwbc.h:251 : q is B x (ndof+1); qdot (B x ndof) may be NULL: only B_, the link
 * velocities and the on-device task reference read it; qddot is accepted for signature parity and unused */
int dwbc_batch_set_state(dwbc_batch *b, const double *q, const double *qdot, const double *qddot);
/* SetContact(bool...) include/dwbc.h:291 : flags is B x n_contacts */
int dwbc_batch_set_contact(dwbc_batch *b, const uint8_t *flags);
/* SetContact with a third flag raised: the reference stacks every flagged contact (src/dwbc.cpp:445-453; its tests register both
 * hands next to the feet, tests/dwbc_test.cpp:68-69).  The product kernels stack two; n = 3 routes every solve of this batch through
 * the general-contact kernel (up to three simultaneously active 6D contacts per instance, hqp = true, tasks on links and on the
 * synthetic "COM" link with f* from SetTaskSpace; trajectories, TASK_CUSTOM levels, the dump record, fp32 and the reduced path are
 * refused at the solve) and widens DWBC_WRENCH to 6 n doubles per instance.  Call before binding a wrench buffer.  n = 2 restores
 * the default. */
int dwbc_batch_set_max_active_contacts(dwbc_batch *b, int n);
int dwbc_batch_max_active_contacts(const dwbc_batch *b);
/* SetTaskSpace(level, f*) include/dwbc.h:333 : fstar is B x task_dof(level) */
int dwbc_batch_set_fstar(dwbc_batch *b, int level, const double *fstar);

/* CopyKinematicsData(target) include/dwbc.h:375, src/dwbc.cpp:1711-1762: state, contact flags, task spaces with their f*, torque
 * limit and control time of `src` into `dst` (same model and batch size); the hand-off the reference uses between threads */
int dwbc_batch_copy_kinematics(dwbc_batch *dst, const dwbc_batch *src);

/* page-locked host mirror of an input field (DWBC_IN_Q, DWBC_IN_CONTACT, DWBC_IN_FSTAR, DWBC_IN_TORQUE; NULL for anything else or before the
 * field has a size): a caller that assembles its states directly in this memory and passes the same pointer to
 * dwbc_batch_set_state / set_contact (or calls dwbc_batch_set_fstar with pointers into it -- level l starts at column
 * fstar offset of l) skips the host-side copy; the upload is one asynchronous PCIe transfer on the batch's stream.
 * Lifetime of the contents: dwbc_batch_solve starts that transfer and returns; the mirror may be REWRITTEN only after the next call
 * of dwbc_batch_host_ptr / dwbc_batch_set_state / set_contact / set_fstar (each waits for the pending upload first) or after
 * dwbc_batch_sync / dwbc_batch_get.  Writing through a pointer kept from before the solve without one of those calls races the DMA. */
void *dwbc_batch_host_ptr(dwbc_batch *b, int field);
/* zero-copy: use a caller-owned DEVICE buffer (e.g. a torch tensor's data_ptr) for an input or output field */
int dwbc_batch_bind_device(dwbc_batch *b, int field, void *device_ptr);
int dwbc_batch_set_stream(dwbc_batch *b, void *hip_stream);
int dwbc_batch_enable_dump(dwbc_batch *b, int on);

/* CalcContactConstraint + CalcGravCompensation + CalcTaskControlTorque(hqp,init) + CalcContactRedistribute(hqp,init)
 * (include/dwbc.h:280,246,349,298) as ONE fused kernel launch on the batch's stream (asynchronous). */
int dwbc_batch_solve(dwbc_batch *b, unsigned flags);
int dwbc_batch_sync(dwbc_batch *b);
/* K back-to-back solves bracketed by HIP events on the batch's stream; returns total milliseconds in *ms */
int dwbc_batch_time_solves(dwbc_batch *b, unsigned flags, int steps, float *ms);
/* copy a field of all B instances to host memory (synchronises the stream) */
int dwbc_batch_get(dwbc_batch *b, int field, void *host_out, size_t bytes);
size_t dwbc_batch_field_bytes(const dwbc_batch *b, int field);
/* kernel launch geometry, for DESIGN.md / bench bookkeeping */
int dwbc_batch_launch_info(const dwbc_batch *b, int *threads_per_instance, int *lds_bytes);
/* name of the kernel the next dwbc_batch_solve will launch (as rocprofv3 prints it), for bench / profile bookkeeping */
const char *dwbc_batch_kernel_name(const dwbc_batch *b);

/* ---- CalcContactRedistribute(torque_input, hqp, init) + getContactForce(torque) for a CALLER-SUPPLIED joint torque (reference
 * include/dwbc.h:297,303, src/dwbc.cpp:1377-1568, src/wbd.cpp:268-271): a torque that came from anywhere -- a policy, a clipped command,
 * another controller -- gets the contact-null-space torque NwJw c that brings the contact wrenches back inside the ZMP / friction rows
 * and the torque limits (DWBC_REDIST_TAU, DWBC_REDIST_CF), and the contact wrench before and after it (DWBC_REDIST_WRENCH).  One lean
 * kernel of its own (kinematics to NwJw and one QP of at most six variables; no task level, no gravity torque): it reads the state, the
 * contact flags and the torque limit of the batch, needs no task space, and leaves DWBC_TAU, DWBC_WRENCH, DWBC_STATUS, DWBC_DIAG, the
 * dump record and the warm-start state of dwbc_batch_solve untouched, so the two may be called on one batch in either order.
 * Per instance: one active contact -> zero torque, status 1 (the wrenches are still evaluated); none -> zeros, status 1; more than two
 * flags raised, a failed contact stage or a failed QP -> status 0, zero torque.
 * Refused (dwbc_last_error): DWBC_F32 batches, dwbc_batch_set_max_active_contacts(b, 3), a model without the kernel (built in for
 * TOCABI's size on its own tree and on any; every kernel pack carries its size's), DWBC_SOLVE_HQP clear (the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque), and a
 * torque input that was never set.  DWBC_SOLVE_INIT clear is accepted and runs cold: the QP is strictly convex, its point does not
 * depend on the start. */
int dwbc_batch_set_torque_input(dwbc_batch *b, const double *tau);   /* B x m; the mirror of dwbc_batch_host_ptr(b, DWBC_IN_TORQUE) is taken in place */
int dwbc_batch_redistribute(dwbc_batch *b, unsigned flags);          /* asynchronous on the batch's stream */
/* K back-to-back redistributions bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_redistribute(dwbc_batch *b, unsigned flags, int steps, float *ms);
/* name of the kernel dwbc_batch_redistribute launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_redistribute_kernel_name(const dwbc_batch *b);

/* ---- CalcGravCompensation() as a call of its own, and ahead of the redistribution (reference include/dwbc.h:246-247,
 * src/dwbc.cpp:875-889, src/wbd.cpp:186-192): the third call of a caller whose torque does not come from the task cascade --
 * UpdateKinematics, SetContact, CalcContactConstraint, CalcGravCompensation, CalcContactRedistribute(torque_grav_ + u), getContactForce --
 * with no task space and one A^-1 sweep per control step.  One lean kernel (the redistribution kernel's stages with torque_grav_ formed
 * from P_C, J_C and the internal-wrench basis; no W, no W^+, no task level) in two forms:
 *   dwbc_batch_grav_compensation(b)                       torque_grav_ and getContactForce(torque_grav_); no torque input, no QP
 *   dwbc_batch_redistribute(b, flags | DWBC_REDIST_ADD_GRAVITY)   the torque input is a command ON TOP OF gravity compensation: the
 *       redistribution of dwbc_batch_redistribute runs on torque_grav_ + torque_input (DWBC_REDIST_WRENCH row 0 is
 *       getContactForce(torque_grav_ + torque_input), row 1 the same after NwJw c), and the three outputs below are written as well.
 *       dwbc_batch_time_redistribute takes the bit too; dwbc_batch_redistribute_kernel_name reports the plain kernel,
 *       dwbc_batch_grav_kernel_name the one either form launches.  Without the bit the three redistribution entry points are what they were.
 * Outputs (buffer slots of their own, no dwbc_field; batch-major):
 *   DWBC_GRAV_TAU (m) f64       torque_grav_
 *   DWBC_GRAV_WRENCH (12) f64   getContactForce(torque_grav_) = Jbar^T[:, 6:] torque_grav_ - P_C, zero padded
 *   DWBC_GRAV_STATUS (1) i32
 * Per instance: one or two active contacts -> torque_grav_, its wrench, status 1; no contact -> zeros, status 1 (torque_grav_ is exactly
 * zero there); more flags raised than two, or a failed contact stage -> zeros, status 0.
 * The launch reads the state, the contact flags and (with the bit) the torque input, the torque limits and the per-instance parameters;
 * it allocates its outputs before its first run and names no output of dwbc_batch_solve, of the plain dwbc_batch_redistribute's inputs
 * beyond those, or of the link query, so all four may be called on one batch in any order.  dwbc_batch_copy_kinematics does not copy it.
 * Refused (dwbc_last_error), in this order: DWBC_F32 batches, dwbc_batch_set_max_active_contacts(b, 3), a model without the kernel (built
 * in for TOCABI's size on its own tree and on any; every kernel pack carries its size's).  With the bit the refusals of
 * dwbc_batch_redistribute come first, with their messages.  dwbc_batch_get_grav before the first launch is refused.
 * Not built: fp32, a third contact, hqp = false (DWBC_SOLVE_HQP clear), the reduced path's ReducedCalcGravCompensation.  The facade's
 * DWBC::RobotData::CalcGravCompensation keeps being served from its cycle. */
enum { DWBC_REDIST_ADD_GRAVITY = 8 };  /* a bit of the `flags` of the three redistribution entry points, beside DWBC_SOLVE_* */
enum dwbc_grav_output { DWBC_GRAV_TAU = 0, DWBC_GRAV_WRENCH = 1, DWBC_GRAV_STATUS = 2 };
int dwbc_batch_grav_compensation(dwbc_batch *b);                  /* asynchronous on the batch's stream */
size_t dwbc_batch_grav_bytes(const dwbc_batch *b, int what);      /* of all B instances; 0: no such output */
int dwbc_batch_get_grav(dwbc_batch *b, int what, void *host_out, size_t bytes);  /* synchronises the stream */
/* zero-copy: a caller-owned DEVICE buffer of dwbc_batch_grav_bytes(b, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_grav(dwbc_batch *b, int what, void *device_ptr);
/* name of the kernel dwbc_batch_grav_compensation launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_grav_kernel_name(const dwbc_batch *b);
/* K back-to-back gravity-only launches bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_grav(dwbc_batch *b, int steps, float *ms);

/* ---- UpdateKinematics as a call of its own (reference include/dwbc.h, src/dwbc.cpp:279-371): what a caller reads between it and
 * SetTaskSpace -- link_[i].xpos / rotm / v / w / jac_ and com_pos -- for a set of queried links, in one lean kernel (forward kinematics;
 * no mass-matrix inverse, no contact stage, no QP).  A query is up to 16 entries (link, point in the link's frame); link =
 * dwbc_model_num_links(m) is the synthetic COM link (com_pos, pelvis rotation, jac_com_, jac_com_ qdot), which takes no point.  Per entry:
 *   DWBC_LQ_POS (3)      p_link + R_link point
 *   DWBC_LQ_ROT (3 x 3)  R_link, row-major
 *   DWBC_LQ_VEL (6)      [v of the point; w]; zero while the state was set without a qdot
 *   DWBC_LQ_JAC (6 x n)  Jacobian of the point, rows [linear; angular] -- the layout dwbc_batch_set_custom_task takes; only if asked for
 * all batch-major: (B, entries, ...).  The launch reads the state alone and names no buffer of dwbc_batch_solve or
 * dwbc_batch_redistribute: their outputs, the dump record and the warm-start state stay as they are, the three may be called on one batch
 * in any order.  dwbc_batch_copy_kinematics does not copy the query.
 * Refused (dwbc_last_error): DWBC_F32 batches and a model without the kernel (built in for TOCABI's size, any tree), both at
 * dwbc_batch_set_link_query; more than 16 entries, a link outside [0, num_links], a COM entry with a non-zero point -- the query and the
 * outputs of the batch stay as they were; dwbc_batch_update_kinematics without a query; DWBC_LQ_JAC of a query set without Jacobians;
 * dwbc_batch_get_link_query before the first launch of the query. */
enum dwbc_link_query_output { DWBC_LQ_POS = 0, DWBC_LQ_ROT = 1, DWBC_LQ_VEL = 2, DWBC_LQ_JAC = 3 };
/* points: n x 3 or NULL (all zero).  n = 0 drops the query.  A new query gets output buffers of its own size: bound ones are let go of
 * (bind again), earlier results are gone. */
int dwbc_batch_set_link_query(dwbc_batch *b, int n, const int32_t *links, const double *points, int want_jacobians);
/* asynchronous on the batch's stream; uploads newer host mirrors of q and qdot first, like a solve */
int dwbc_batch_update_kinematics(dwbc_batch *b);
size_t dwbc_batch_link_query_bytes(const dwbc_batch *b, int what);  /* of all B instances; 0: no query, no such output */
int dwbc_batch_get_link_query(dwbc_batch *b, int what, void *host_out, size_t bytes);  /* synchronises the stream */
/* zero-copy: a caller-owned DEVICE buffer of dwbc_batch_link_query_bytes(b, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_link_query(dwbc_batch *b, int what, void *device_ptr);
/* name of the kernel dwbc_batch_update_kinematics launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_link_query_kernel_name(const dwbc_batch *b);

/* ---- the dynamics half of UpdateKinematics as a call of its own (reference src/dwbc.cpp:279-371): what a caller reads off RobotData
 * after it -- rd_.A_, A_inv_, B_, G_, CMM_, com_pos (the reference's harnesses: torque = A_.bottomRows(m) jacc + J_C^T f + B_.tail(m),
 * y = -A_inv_ B_, CMM_ q_dot) -- in one lean kernel (stage 0 of the cycle: kinematics, CRBA, the A^-1 sweep; the RNEA of B_; the centroidal
 * block.  No contact stage, no task level, no QP).  The caller asks for a set of outputs; what is not asked for is not computed:
 * without DWBC_DYN_A_INV there is no sweep, without DWBC_DYN_B (or without a qdot) no RNEA, without DWBC_DYN_CMM / DWBC_DYN_COM no
 * centroidal block.  Outputs (buffer slots of their own, no dwbc_field; batch-major):
 *   DWBC_DYN_A (n, n) f64       A_
 *   DWBC_DYN_A_INV (n, n) f64   A_inv_
 *   DWBC_DYN_B (n) f64          B_ = C qdot + g; while the state was set without a qdot, G_ to the bit (B_(q, 0) = G_)
 *   DWBC_DYN_G (n) f64          G_
 *   DWBC_DYN_CMM (6, n) f64     CMM_
 *   DWBC_DYN_COM (3) f64        com_pos
 *   DWBC_DYN_STATUS (1) i32     always written; 0 only if DWBC_DYN_A_INV was asked for and the sweep met a pivot that is not positive:
 *                               every asked-for output of that instance is then zero
 * The launch reads the state and the model alone: it needs no contact and no task space, dwbc_batch_set_max_active_contacts does not
 * matter to it, and it names no buffer of dwbc_batch_solve, dwbc_batch_redistribute, dwbc_batch_grav_compensation or the link query --
 * their outputs, the dump record and the warm-start state stay as they are, and all five may be called on one batch in any order.
 * dwbc_batch_copy_kinematics does not copy the request.
 * Refused (dwbc_last_error): DWBC_F32 batches, then a model without the kernel (built in for TOCABI's size on its own tree and on any;
 * every kernel pack carries its size's), both at dwbc_batch_set_dynamics_outputs; an unknown bit -- the request and the outputs of the
 * batch stay as they were; dwbc_batch_update_dynamics without a request; get / bind of an output that was not asked for;
 * dwbc_batch_get_dynamics before the first launch of the request.
 * Not built: fp32; the facade include/dwbc_amd.hpp, which keeps mirroring these members from its cycle; jac_com_ and the COM inertia (the
 * link query's COM entry serves jac_com_); products such as A qddot + B; the reduced model's matrices; the link query in kernel packs. */
enum dwbc_dynamics_output { DWBC_DYN_A = 0, DWBC_DYN_A_INV = 1, DWBC_DYN_B = 2, DWBC_DYN_G = 3, DWBC_DYN_CMM = 4, DWBC_DYN_COM = 5, DWBC_DYN_STATUS = 6 };
/* mask: bits 1u << dwbc_dynamics_output; DWBC_DYN_STATUS is implied.  0 drops the request and its buffers.  A new request gets output
 * buffers of its own: bound ones are let go of (bind again), earlier results are gone. */
int dwbc_batch_set_dynamics_outputs(dwbc_batch *b, unsigned mask);
/* asynchronous on the batch's stream; uploads newer host mirrors of q and qdot first, like a solve */
int dwbc_batch_update_dynamics(dwbc_batch *b);
size_t dwbc_batch_dynamics_bytes(const dwbc_batch *b, int what);  /* of all B instances; 0: not asked for, no such output */
int dwbc_batch_get_dynamics(dwbc_batch *b, int what, void *host_out, size_t bytes);  /* synchronises the stream */
/* zero-copy: a caller-owned DEVICE buffer of dwbc_batch_dynamics_bytes(b, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_dynamics(dwbc_batch *b, int what, void *device_ptr);
/* name of the kernel dwbc_batch_update_dynamics launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_dynamics_kernel_name(const dwbc_batch *b);
/* K back-to-back launches of the request bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_dynamics(dwbc_batch *b, int steps, float *ms);

/* ---- SetContact + CalcContactConstraint as a call of its own (reference include/dwbc.h:432-474, src/dwbc.cpp:433-478,
 * src/wbd.cpp:108-143): the contact-space members a caller reads off RobotData between UpdateKinematics and SetTaskSpace (the reference's
 * harnesses: J_t A_inv_ N_C for a task acceleration, J_C^T f in an inverse-dynamics check; tests/dwbc_test.cpp:92-113 pins seven of them)
 * in one lean kernel: stage 0 of the cycle, its contact stage, the NwJw closed form and the W^+ sweep.  No task level, no gravity vector,
 * no QP.  The caller asks for a set of outputs; what is not asked for is not computed: only J_C and / or the contact frames -- no A^-1
 * sweep; none of A_INV_N_C, W, W_INV -- the columns are never updated to A^-1 N_c; no W_INV -- no W + alpha P and no 33-pivot sweep;
 * neither NWJW nor W_INV -- no internal-wrench basis; no N_C -- no n x n product.  Outputs (buffer slots of their own, no dwbc_field;
 * batch-major; the shapes are fixed whatever the support, zero beyond the active contact dof cd; m = n - 6):
 *   DWBC_CS_J_C (12, n) f64          J_C               src/dwbc.cpp:445-453
 *   DWBC_CS_LAMBDA_C (12, 12) f64    Lambda_contact    src/wbd.cpp:115   row stride 12, zero outside cd x cd (the dump field DWBC_LAMBDA_C has stride cd)
 *   DWBC_CS_J_C_INV_T (12, n) f64    J_C_INV_T         src/wbd.cpp:116
 *   DWBC_CS_N_C (n, n) f64           N_C               src/wbd.cpp:117
 *   DWBC_CS_A_INV_N_C (n, n) f64     A_inv_N_C         src/wbd.cpp:118
 *   DWBC_CS_W (m, m) f64             W                 src/wbd.cpp:119
 *   DWBC_CS_W_INV (m, m) f64         W_inv             src/wbd.cpp:124, 140
 *   DWBC_CS_NWJW (m, 6) f64          NwJw              src/wbd.cpp:128   zero on one foot (k = 0)
 *   DWBC_CS_CONTACT_POS (2, 3) f64   cc_[i].xc_pos     in the order of the active contacts, as DWBC_CONTACT_POS
 *   DWBC_CS_CONTACT_ROT (2, 9) f64   cc_[i].rotm
 *   DWBC_CS_STATUS (1) i32           return value of CalcContactConstraint; always written
 * Support: both feet (k = 6); one foot (k = 0: W has full rank, W_inv is its inverse); no active contact (N_C = I, A_inv_N_C = A_inv,
 * W its joint block, W_inv that block's inverse, every contact-sized output zero, status 1).  More flags set than two (device-resident
 * flags), a failed Lambda_c or a bad pivot of the W sweep: status 0 and every asked-for output of that instance zero.
 * The launch reads the state, the model, the registered contacts and the flags: it needs no task space, reads no f*, torque limit or
 * per-instance parameter record, and names no buffer of dwbc_batch_solve, dwbc_batch_redistribute, dwbc_batch_grav_compensation,
 * dwbc_batch_update_kinematics or dwbc_batch_update_dynamics -- the six may be called on one batch in any order.
 * Refused (dwbc_last_error), in this order, before anything is launched: DWBC_F32 batches; dwbc_batch_set_max_active_contacts above 2; a
 * model without the kernel (built in for TOCABI's size on its own tree and on any; every kernel pack carries its size's); a batch without a
 * registered contact -- all four at dwbc_batch_set_contact_space_outputs already.  Further: an unknown bit; a launch without a request;
 * get / bind of an output that was not asked for; dwbc_batch_get_contact_space before the first launch of the request.
 * Not built: three contacts, fp32, the reduced system's matrices, V2 (the device forms NwJw in closed form and has no COD basis), P_C (an
 * output of the gravity launch's arithmetic); the facade include/dwbc_amd.hpp keeps serving these members from its cycle. */
enum dwbc_contact_space_output {
    DWBC_CS_J_C = 0, DWBC_CS_LAMBDA_C = 1, DWBC_CS_J_C_INV_T = 2, DWBC_CS_N_C = 3, DWBC_CS_A_INV_N_C = 4, DWBC_CS_W = 5, DWBC_CS_W_INV = 6,
    DWBC_CS_NWJW = 7, DWBC_CS_CONTACT_POS = 8, DWBC_CS_CONTACT_ROT = 9, DWBC_CS_STATUS = 10
};
/* mask: bits 1u << dwbc_contact_space_output; DWBC_CS_STATUS is implied.  0 drops the request and its buffers.  A new request gets output
 * buffers of its own: bound ones are let go of (bind again), earlier results are gone. */
int dwbc_batch_set_contact_space_outputs(dwbc_batch *b, unsigned mask);
/* SetContact (with the flags of dwbc_batch_set_contact, or device-bound DWBC_IN_CONTACT) + CalcContactConstraint; asynchronous on the
 * batch's stream; uploads newer host mirrors of q and the contact flags first, like a solve */
int dwbc_batch_calc_contact_constraint(dwbc_batch *b);
size_t dwbc_batch_contact_space_bytes(const dwbc_batch *b, int what);  /* of all B instances; 0: not asked for, no such output */
int dwbc_batch_get_contact_space(dwbc_batch *b, int what, void *host_out, size_t bytes);  /* synchronises the stream */
/* zero-copy: a caller-owned DEVICE buffer of dwbc_batch_contact_space_bytes(b, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_contact_space(dwbc_batch *b, int what, void *device_ptr);
/* name of the kernel dwbc_batch_calc_contact_constraint launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_contact_space_kernel_name(const dwbc_batch *b);
/* K back-to-back launches of the request bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_contact_space(dwbc_batch *b, int steps, float *ms);

/* ---- SetTaskSpace + CalcTaskSpace as a call of its own (reference src/dwbc.cpp:795-816, src/task.cpp:90-93,202-211,
 * src/wbd.cpp:207-261): what a caller reads off ts_[i] between CalcTaskSpace and a torque law of its own (the reference's harnesses:
 * Null_task_[i-1] J_kt_ Lambda_task_ f_star_ in tests/sp_test/redu_dyn_test.cpp) in one lean kernel: the contact-space launch's front and,
 * per task level, the matrices of the restatement's level loop.  No f*, no trajectory, no QP.  The caller asks for a set of outputs; what is
 * not asked for is not computed: only J_TASK -- nothing behind the kinematics; neither J_KT nor NULL_TASK -- nothing behind Lambda_task; no
 * NULL_TASK -- no projector, no m x m store.  Outputs per level (buffer slots of their own, no dwbc_field and no output of a
 * dwbc_lean_family; batch-major; t = dwbc_batch_task_dof(b, level), m = n - 6):
 *   DWBC_TS_J_TASK (t, n) f64        ts_[level].J_task_
 *   DWBC_TS_LAMBDA_TASK (t, t) f64   ts_[level].Lambda_task_
 *   DWBC_TS_J_KT (m, t) f64          ts_[level].J_kt_
 *   DWBC_TS_NULL_TASK (m, m) f64     ts_[level].Null_task_     every level but the last (the reference forms none there, src/dwbc.cpp:804)
 *   DWBC_TS_STATUS (1) i32           one per instance, whatever `level` is; always written
 * Status 0 -- more flags set than two (device-resident flags), a failed Lambda_c, a bad pivot of the W sweep, or a t x t block of some
 * level that the small inverses reject -- and every asked-for output of that instance is zero.  No active contact is served.
 * The launch reads the state, the model, the registered contacts, the flags and the task levels, and names no buffer of dwbc_batch_solve
 * or of the other lean launches.  dwbc_batch_add_task / _add_custom_task / _clear_tasks drop the request (the shapes follow the levels).
 * Refused (dwbc_last_error), in this order, before anything is launched: DWBC_F32 batches; dwbc_batch_set_max_active_contacts above 2; a
 * level of more than 6 dof; a TASK_CUSTOM level; a model without the kernel (built in for TOCABI's size on its own tree and on any; every
 * kernel pack carries its size's); a batch without a task level -- all six at dwbc_batch_set_task_space_outputs already.  Further: an
 * unknown bit; a launch without a request; get / bind of an output that was not asked for, of a level that does not exist, or of
 * NULL_TASK of the last level; a get before the first launch of the request; a wrong byte count.
 * Not built: three contacts, fp32, TASK_CUSTOM levels, levels wider than 6 dof, f* and trajectories (the cycle keeps UpdateTaskSpace);
 * the facade include/dwbc_amd.hpp keeps serving ts_[i] from its cycle. */
enum dwbc_task_space_output { DWBC_TS_J_TASK = 0, DWBC_TS_LAMBDA_TASK = 1, DWBC_TS_J_KT = 2, DWBC_TS_NULL_TASK = 3, DWBC_TS_STATUS = 4 };
/* output `index` of the launch for a model of n dof and a level of t task dof, as dwbc_lean_output_describe answers for the families;
 * 0 when index is past the end.  Needs no device and no batch. */
int dwbc_task_space_output_describe(int index, int n, int t, dwbc_field_info *out);
/* mask: bits 1u << dwbc_task_space_output; DWBC_TS_STATUS is implied.  0 drops the request and its buffers.  Plans at once and allocates
 * every output of every level, so that the launch allocates nothing; bound buffers are let go of (bind again), earlier results are gone. */
int dwbc_batch_set_task_space_outputs(dwbc_batch *b, unsigned mask);
/* one launch, asynchronous on the batch's stream; uploads newer host mirrors of q and the contact flags first, like a solve */
int dwbc_batch_calc_task_space(dwbc_batch *b);
size_t dwbc_batch_task_space_bytes(const dwbc_batch *b, int level, int what);  /* of all B instances; 0: not asked for, no such output */
/* synchronises the stream; bytes must be dwbc_batch_task_space_bytes(b, level, what) */
int dwbc_batch_get_task_space(dwbc_batch *b, int level, int what, void *host_out, size_t bytes);
/* zero-copy: a caller-owned DEVICE buffer of dwbc_batch_task_space_bytes(b, level, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_task_space(dwbc_batch *b, int level, int what, void *device_ptr);
/* name of the kernel dwbc_batch_calc_task_space launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_task_space_kernel_name(const dwbc_batch *b);
/* K back-to-back launches of the request bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_task_space(dwbc_batch *b, int steps, float *ms);

/* ---- RobotData::CalcSingleTaskTorqueWithQP(ts, task_null_matrix, torque_prev, NwJw, J_C_INV_T, P_C, init) as a call of its own (reference
 * include/dwbc.h:354, src/dwbc.cpp:941-1127): the constrained solve of ONE task level, the step CalcTaskControlTorque takes once per level
 * (src/dwbc.cpp:830-852), for a caller that closes its own hierarchy law -- reorders or skips levels, puts a level beneath a torque of its
 * own, or mixes its own projector into the chain.  One launch is one call of the method on every instance:
 *   inputs    the level; torque_prev (m), required; task_null_matrix (m, m) row-major, optional: absent means the identity, as the
 *             reference passes for level 0; f* of the level is the batch's own (dwbc_batch_set_fstar / bound DWBC_IN_FSTAR); the state, the
 *             contact flags, the torque limit, the contact constants and the per-instance parameters are the batch's
 *   computed  NwJw, J_C_INV_T, P_C, J_kt and Lambda_task from the state; Ntorque_task = N J_kt Lambda_task; the QP in [f_star_qp (t);
 *             contact_qp (k)], k = max(contact dof - 6, 0), with the rows of src/dwbc.cpp:1001-1053 (2 m torque rows only with a torque limit,
 *             10 cone rows per active contact), started cold, solved by the cycle's solver under the cycle's canon
 * Outputs per instance (buffer slots of their own; batch-major; m = n - 6):
 *   DWBC_TQ_F_STAR_QP (6) f64         ts.f_star_qp_, zero beyond t
 *   DWBC_TQ_CONTACT_QP (6) f64        ts.contact_qp_, zero beyond k
 *   DWBC_TQ_TORQUE_H (m) f64          J_kt Lambda (f* + f_star_qp)              (src/dwbc.cpp:839)
 *   DWBC_TQ_TORQUE_NULL_H (m) f64     N torque_h: what is added to torque_task_ (:840, :849)
 *   DWBC_TQ_TORQUE_CONTACT (m) f64    NwJw contact_qp, zero when k = 0         (:851)
 *   DWBC_TQ_STATUS (1) i32            always written
 * Status 1: the QP solved.  0: the reference's failure (src/dwbc.cpp:1117-1125) and whatever makes the task-space launch answer 0 -- more
 * flags set than two (device-resident flags), a failed Lambda_c, a bad pivot of the W sweep, a rejected t x t block -- and every other
 * output of that instance is zero.
 * The launch names no buffer of dwbc_batch_solve or of the other lean launches.  dwbc_batch_add_task / _add_custom_task / _clear_tasks drop
 * the request and the inputs.
 * Refused (dwbc_last_error), in this order, before anything is launched: DWBC_F32 batches; dwbc_batch_set_max_active_contacts above 2; a
 * level of more than 6 dof; a TASK_CUSTOM level; a model without the kernel (built in for TOCABI's size on its own tree and on any; kernel
 * packs do not carry one); a batch without a task level -- all six at dwbc_batch_set_task_qp already.  Further: an unknown bit; a level out
 * of range; a level that carries a trajectory (its f* is formed on the device, not read from DWBC_IN_FSTAR); a launch without a request or
 * without torque_prev; a bound buffer or a host buffer of the wrong size; dwbc_batch_set_task_qp_inputs on an input that is bound; get / bind
 * of an output that was not asked for; a get before the first launch of the request.
 * Not built: kernel packs, fp32, three contacts, levels wider than 6 dof, TASK_CUSTOM levels, warm starts, the reduced path, the facade. */
enum dwbc_task_qp_output {
    DWBC_TQ_F_STAR_QP = 0, DWBC_TQ_CONTACT_QP = 1, DWBC_TQ_TORQUE_H = 2, DWBC_TQ_TORQUE_NULL_H = 3, DWBC_TQ_TORQUE_CONTACT = 4, DWBC_TQ_STATUS = 5
};
enum dwbc_task_qp_input { DWBC_TQ_IN_TORQUE_PREV = 0, DWBC_TQ_IN_NULL = 1 };
/* output `index` of the launch for a model of n dof, as dwbc_lean_output_describe answers for the families; 0 when index is past the end.
 * Needs no device and no batch. */
int dwbc_task_qp_output_describe(int index, int n, dwbc_field_info *out);
/* the level and mask: bits 1u << dwbc_task_qp_output; DWBC_TQ_STATUS is implied.  mask 0 drops the request and its output buffers.  Plans at
 * once and allocates every output, so that the launch allocates nothing; bound outputs are let go of (bind again), earlier results are gone;
 * the inputs stay */
int dwbc_batch_set_task_qp(dwbc_batch *b, int level, unsigned mask);
/* torque_prev: B x m; null: B x m x m or NULL (the identity; a null matrix set or bound before is let go of).  A host copy into a page-locked
 * mirror, uploaded with the next launch */
int dwbc_batch_set_task_qp_inputs(dwbc_batch *b, const double *torque_prev, const double *null_or_NULL);
/* zero-copy: a caller-owned DEVICE buffer for one input (which: dwbc_task_qp_input) of exactly `bytes` = B m 8 (torque_prev) or B m m 8
 * (null) bytes; device_ptr NULL lets go of the input (the null matrix: back to the identity) */
int dwbc_batch_bind_task_qp_input(dwbc_batch *b, int which, void *device_ptr, size_t bytes);
/* one launch, asynchronous on the batch's stream; uploads newer host mirrors of q, the contact flags, f*, the per-instance parameters and the
 * two inputs first, like a solve */
int dwbc_batch_calc_single_task_torque_qp(dwbc_batch *b);
size_t dwbc_batch_task_qp_bytes(const dwbc_batch *b, int what);  /* of all B instances; 0: not asked for, no such output */
/* synchronises the stream; bytes must be dwbc_batch_task_qp_bytes(b, what) */
int dwbc_batch_get_task_qp(dwbc_batch *b, int what, void *host_out, size_t bytes);
/* zero-copy: a caller-owned DEVICE buffer of `bytes` = dwbc_batch_task_qp_bytes(b, what) bytes for one output; NULL: back to the batch's own */
int dwbc_batch_bind_task_qp(dwbc_batch *b, int what, void *device_ptr, size_t bytes);
/* name of the kernel dwbc_batch_calc_single_task_torque_qp launches on this batch ("" and dwbc_last_error when it would be refused) */
const char *dwbc_batch_task_qp_kernel_name(const dwbc_batch *b);
/* K back-to-back launches of the request bracketed by HIP events, as dwbc_batch_time_solves */
int dwbc_batch_time_task_qp(dwbc_batch *b, int steps, float *ms);

/* ---- generic hierarchical-QP class for a batch: DWBC::HQP / HQP_Hierarch (reference include/dwbc_hqp.h:8-141,
 * src/dwbc_hqp.cpp).  Every level i poses  A_i y + a_i <= v (inequalities with slack), B_i y + b_i = w (equalities, least
 * squares), optional cost 1/2 y^T H y; levels are solved in sequence inside the null space of the earlier equalities.  The
 * reference solves each level with OSQP (not vendored); here each level is solved exactly on the device (DESIGN.md "HQP
 * class").  All matrices are per instance, batch-major, row-major: A is B x ineq x nv, nv = acceleration + torque + contact. */
typedef struct dwbc_hqp dwbc_hqp;
enum dwbc_hqp_field {
    DWBC_HQP_Y_ANS = 0,   /* (nv)   f64  hqp_hs_[level].y_ans_ */
    DWBC_HQP_V_ANS = 1,   /* (ineq) f64  hqp_hs_[level].v_ans_ */
    DWBC_HQP_W_ANS = 2,   /* (eq)   f64  hqp_hs_[level].w_ans_ = B y + b */
    DWBC_HQP_STATUS = 3,  /* (1)    i32  1 solved / 0 failed (iteration limit, working set overflow, singular Hessian) */
    DWBC_HQP_ITER = 4,    /* (1)    i32  active-set steps of the level */
    DWBC_HQP_NULL_SIZE = 5, /* (1)  i32  hqp_hs_[level].null_space_size_ */
    DWBC_HQP_A = 6, DWBC_HQP_a = 7, DWBC_HQP_B = 8, DWBC_HQP_b = 9  /* the (normalised) level matrices as stored */
};
dwbc_hqp *dwbc_hqp_create(int B, int device, int acceleration_size, int torque_size, int contact_size); /* HQP::initialize :16-21 */
void dwbc_hqp_destroy(dwbc_hqp *h);
int dwbc_hqp_add_hierarchy(dwbc_hqp *h, int ineq_const_size, int eq_const_size);   /* HQP::addHierarchy :425-434; returns the level */
int dwbc_hqp_clear(dwbc_hqp *h);                                                    /* drop every level */
/* HQP_Hierarch::updateConstraintMatrix :530-547 (A, a may be NULL for a level without inequalities) */
int dwbc_hqp_update_constraint_matrix(dwbc_hqp *h, int level, const double *A, const double *a, const double *Bm, const double *b);
int dwbc_hqp_update_cost_matrix(dwbc_hqp *h, int level, const double *H, const double *g);  /* updateCostMatrix :483-493 (g is stored, never read: as in the reference) */
int dwbc_hqp_normalize_constraint_matrix(dwbc_hqp *h, int level);                   /* normalizeConstraintMatrix :555-581 */
/* HQP_Hierarch::updateInequalityCostWeight / updateEqualityCostWeight / updateConstraintWeight :503-553.  V: B x ineq x ineq, W: B x eq x eq
 * (row major per instance; NULL = identity).  As in the reference they enter dwbc_hqp_solve_first only (level 0 posed on V A, V a, W B,
 * W b, :245-254); solveSequential reads the unweighted matrices, and the weights of later levels are stored and never read. */
int dwbc_hqp_update_constraint_weight(dwbc_hqp *h, int level, const double *V, const double *W);
/* seed hqp_hs_[level].y_ans_ / v_ans_ directly, as ConfigureLQP does for level 0 (src/dwbc.cpp:4378-4381) */
int dwbc_hqp_set_answer(dwbc_hqp *h, int level, const double *y_ans, const double *v_ans);
int dwbc_hqp_prepare(dwbc_hqp *h);                    /* HQP::prepare :23-85 (the null-space chain itself is evaluated with the solve) */
int dwbc_hqp_solve_first(dwbc_hqp *h, int init);      /* HQP::solvefirst :222-289 */
int dwbc_hqp_solve_sequential(dwbc_hqp *h, int init); /* HQP::solveSequential :397-403; init is accepted and unused (exact solves have no warm state) */
int dwbc_hqp_num_levels(const dwbc_hqp *h);
size_t dwbc_hqp_field_bytes(const dwbc_hqp *h, int level, int field);
int dwbc_hqp_get(dwbc_hqp *h, int level, int field, void *host_out, size_t bytes);
/* RobotData::ConfigureLQP(hqp) src/dwbc.cpp:4304-4430 on the device, from the batch's last solve (needs dwbc_batch_enable_dump and
 * the same contact flags in every instance): (re)builds the levels of `h` -- torque limit / floating-base dynamics,
 * contact cones + acceleration limit / contact constraint, one equality level per task space -- and seeds level 0.
 * RobotData::CalcControlTorqueLQP(hqp) src/dwbc.cpp:4432-4452 is dwbc_hqp_solve_sequential(h, init). */
int dwbc_batch_configure_lqp(dwbc_batch *b, dwbc_hqp *h);
/* torque of the LQP answer, tau = A[6:] qddot + J_C^T[6:] f_c + B_[6:] (tests/sp_test/jacc_compare.cpp:416-418): B x m */
int dwbc_batch_lqp_torque(dwbc_batch *b, dwbc_hqp *h, double *tau);
/* RobotData::CalcSingleTaskTorqueWithJACC_QP(ts_[level], init) src/dwbc.cpp:3772-3945: the joint-acceleration QP of one task level
 * (variables qddot, tau, f_c and the task slack; dynamics, contact and the earlier levels' tasks as equalities; contact cones,
 * |qddot_joint| <= 10, |tau| <= 200) from the batch's last solve (dump on, one contact state per batch), solved exactly on `h`
 * (which is rebuilt for it).  Levels must be solved in order: level i uses f*_qp of the levels before it.  Results per instance:
 * ts_[level].acc_qp_ (ndof), torque_qp_ (m), contact_qp_ (12, zero padded), f_star_qp_ (6, zero padded), status (i32) */
enum dwbc_jacc_field { DWBC_JACC_ACC = 0, DWBC_JACC_TORQUE = 1, DWBC_JACC_CONTACT = 2, DWBC_JACC_FSTAR_QP = 3, DWBC_JACC_STATUS = 4 };
int dwbc_batch_solve_jacc(dwbc_batch *b, dwbc_hqp *h, int level);
int dwbc_batch_get_jacc(dwbc_batch *b, int level, int field, void *host_out, size_t bytes);

/* ---- the same formulations on the REDUCED system, after a cycle solved with DWBC_SOLVE_REDUCED (dump on, one contact state per
 * batch).  RS = vc_dof + 6 (24 for TOCABI double support): contact-chain coordinates + 6 centroidal coordinates of the other bodies.
 * The contact-chain task levels (`!noncont_task`) are taken in level order; `level` below counts THEM.
 *   RobotData::ConfigureLQP_R(hqp)            src/dwbc.cpp:4504-4632  (A_R, J_CR, G_R, J_task J_R_INV_T^T; cost scaled by |A_|_F of
 *                                              the full model; torque limit 200, 600 on row RS-6-4).  HQP sizes (RS, 0, contact dof).
 *   RobotData::CalcControlTorqueLQP_R(hqp)    :4455-4477 = dwbc_hqp_solve_sequential.  dwbc_batch_lqp_torque then returns
 *                                              B x (RS-6): the 12 / 6 chain torques and the wrench on the centroidal coordinates.
 *   CalcSingleTaskTorqueWithJACC_QP_R         :3946-4122 (|tau| <= 200 on the chain joints only); results through dwbc_batch_get_jacc
 *                                              with acc_qp_ (RS) and torque_qp_ (RS-6).
 * The non-contact halves take ONE 6-D task level on a non-contact link (the reference reads ts_[1] as such); `level` is the task level
 * as registered.  HQP sizes (nc_dof, 0, 0), nc_dof = ndof - vc_dof.
 *   RobotData::ConfigureLQP_R_NC(hqp_nc, q_acc) :4634-4760: q_acc = the last level's answer of the solved reduced LQP `hr`.  Then
 *                                              CalcControlTorqueLQP_R_NC :4479-4502 = dwbc_hqp_solve_first + dwbc_hqp_solve_sequential.
 *   CalcSingleTaskTorqueWithJACC_QP_R_NC(ts, prev_acc) :4124-4302: prev_acc = acc_qp_ of the reduced JACC level `src_level`.  Results
 *                                              (dwbc_batch_get_jacc_nc): acc_qp_ (nc_dof), torque_qp_ (nc_dof), gacc_qp_ (6, under
 *                                              DWBC_JACC_CONTACT), f_star_qp_ (6), status. */
/* vc_dof and nc_dof of the contact state set through dwbc_batch_set_contact (src/dwbc.cpp:2818-2823); 0 if the contact chains
 * do not occupy the leading joint dofs (the reduced path's scope) */
int dwbc_batch_reduced_dims(dwbc_batch *b, int *vc_dof, int *nc_dof);
int dwbc_batch_configure_lqp_r(dwbc_batch *b, dwbc_hqp *h);
int dwbc_batch_configure_lqp_r_nc(dwbc_batch *b, dwbc_hqp *h_nc, const dwbc_hqp *hr, int level);
int dwbc_batch_solve_jacc_r(dwbc_batch *b, dwbc_hqp *h, int level);
int dwbc_batch_solve_jacc_r_nc(dwbc_batch *b, dwbc_hqp *h_nc, int level, int src_level);
int dwbc_batch_get_jacc_nc(dwbc_batch *b, int field, void *host_out, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
