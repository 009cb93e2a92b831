// emu_task_qp.cpp -- TEST HARNESS ONLY.  The single-level task-QP kernel source (libdwbc_amd/csrc/dwbc_task_qp.h) compiled for the host with
// one "thread" per workgroup (NT = 1, barriers are no-ops): TOCABI's size (39, 34) on its constant tree and on TopoGeneric.  A translation
// unit of its own: one entry point, the model given as arrays, one run described by its arguments.  LDS is exactly LdsTq<N, NB>::total doubles,
// NaN-poisoned before every instance, with a guard behind it that must come back untouched.  Loaded by tests/emu/emu_task_qp.py.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_task_qp.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

namespace {
constexpr int kGuard = 256;

template <int N, int NB, class Topo>
int run_size(const Setup &su, const BatchIO &io, const TqIO &qio, std::string &err) {
    const int total = LdsTq<N, NB>::total;
    std::vector<real_t> lds((size_t)total + kGuard);
    const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
    for (int b = 0; b < io.B; b++) {
        std::fill(lds.begin(), lds.begin() + total, nan);
        std::fill(lds.begin() + total, lds.end(), real_t(-7.0));
        task_qp_instance<N, NB, 1, Topo>(Thr{0}, su, io, qio, b, lds.data());
        for (int i = total; i < total + kGuard; i++)
            if (!(lds[i] == real_t(-7.0))) {
                err = "write behind the end of the LDS map at double " + std::to_string(i) + " of " + std::to_string(total);
                return 0;
            }
    }
    return 1;
}
}  // namespace

extern "C" {

// total_bytes of the map at one of the sizes; 0: not listed
int emu_task_qp_lds_bytes(int n) {
    switch (n) {
    case 23: return LdsTq<23, 18>::total_bytes;
    case 37: return LdsTq<37, 32>::total_bytes;
    case 39: return LdsTq<39, 34>::total_bytes;
    case 43: return LdsTq<43, 38>::total_bytes;
    case 50: return LdsTq<50, 45>::total_bytes;
    }
    return 0;
}

// model, contacts (with lx ly mu muz per contact in c_par) and task links: as emu_task_space_run.  tau_lim: M limits or NULL (no torque
// rows); inst_par: B x (M + 4 nc) or NULL.  fstar: B x fstar_total; torque_prev: B x M; null: B x M x M or NULL.  mask: bits
// 1u << dwbc_task_qp_output (the status is always written).  out: five pointers in the order of the enum; one that is not written may be NULL.
int emu_task_qp_run(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                    const double *inertia, int nc, const int *c_link, const double *c_point, const double *c_par, int nt, const int *t_level,
                    const int *t_mode, const int *t_link, const double *t_point, const double *tau_lim, const double *inst_par, int B,
                    const double *q, const unsigned char *flags, const double *fstar, int level, const double *torque_prev, const double *null,
                    unsigned mask, int tree, double *const *out, int *status, char *err, int err_len) {
    auto fail = [&](const std::string &s) {
        strncpy(err, s.c_str(), (size_t)err_len - 1);
        err[err_len - 1] = 0;
        return 0;
    };
    Model m;
    m.parent.assign(parent, parent + nb);
    m.R_T.assign(R_T, R_T + 9 * nb);
    m.p_T.assign(p_T, p_T + 3 * nb);
    m.axis.assign(axis, axis + 3 * nb);
    m.mass.assign(mass, mass + nb);
    m.com.assign(com, com + 3 * nb);
    m.inertia.assign(inertia, inertia + 9 * nb);
    for (int i = 0; i < nb; i++) m.names.push_back("link" + std::to_string(i));
    m.finalize();
    Setup su;
    setup_init(su, m.nb, m.ndof, m.maxdepth);
    std::vector<double> body;
    std::vector<int> topo;
    m.body_table(body);
    m.topo_table(topo);
    setup_set_parents(su, topo.data());
    std::string e;
    for (int i = 0; i < nc; i++)
        if (setup_add_contact(su, c_link[i], 0, c_point + 3 * i, c_par[4 * i], c_par[4 * i + 1], c_par[4 * i + 2], c_par[4 * i + 3], e) < 0) return fail(e);
    for (int i = 0; i < nt; i++)
        if (!setup_add_task(su, t_level[i], t_mode[i], t_link[i], t_point + 3 * i, e)) return fail(e);
    if (su.n_levels < 1 || setup_wide_tasks(su)) return fail("emu_task_qp: 1 to 4 levels of at most 6 dof");
    if (level < 0 || level >= su.n_levels) return fail("emu_task_qp: no such level");
    if (tau_lim) {
        su.has_tau_lim = 1;
        for (int i = 0; i < m.ndof - 6; i++) su.tau_lim[i] = tau_lim[i];
    }
    if (inst_par) su.has_tau_lim = 1;  // as launch_setup of dwbc_capi.hip: with a per-instance record the torque rows exist
    BatchIO io{};  // the state, the flags, f* and the model: every other pointer stays NULL, so a read of one faults here
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar;
    io.body = body.data();
    io.topo = topo.data();
    io.hqp = 1;
    io.pair_swap_bit = -1;
    io.inst_par = inst_par;
    TqIO qio{};
    qio.mask = mask;
    qio.level = level;
    qio.torque_prev = torque_prev;
    qio.null = null;
    qio.f_star_qp = out[0];
    qio.contact_qp = out[1];
    qio.torque_h = out[2];
    qio.torque_null_h = out[3];
    qio.torque_contact = out[4];
    qio.status = status;
    qio.cs_mask = kTqContactStageMask;  // as dwbc_capi.hip launches it; cs_out stays NULL, so a store through it faults here
    if (m.ndof != 39 || nb != 34) return fail("emu_task_qp is instantiated for (39, 34)");
    if (tree) {
        if (su.topo_kind != 1) return fail("emu_task_qp: the constant tree is TOCABI's");
        return run_size<39, 34, TopoTocabi>(su, io, qio, e) ? 1 : fail(e);
    }
    return run_size<39, 34, TopoGeneric>(su, io, qio, e) ? 1 : fail(e);
}
}
