// emu_inst_model.cpp -- TEST HARNESS ONLY.  The cycle kernels (libdwbc_amd/csrc/dwbc_cycle2.h, dwbc_cycle2p.h) and the dynamics kernel
// (dwbc_dynamics.h) compiled for the host under DWBC_INST_MODEL, as the dwbc_im:: build of the library compiles them: BatchIO::body holds
// one body table per instance and DWBC_BODY (dwbc_types.h) picks the instance's own.  One "thread" per workgroup (NT = 1, barriers are
// no-ops), TOCABI's size on its constant tree.  A translation unit of its own: the model's tree given as arrays, the tables as
// B x nb x 25 doubles, one run described by its arguments.  LDS is NaN-poisoned before every instance.  Loaded by
// tests/emu/emu_inst_model.py, which also builds it with DWBC_BODY predefined to a wrong expression (the mutants of
// tests/test_instance_model_emu.py).
#define DWBC_HOST_EMU 1
#ifndef DWBC_INST_MODEL
#error "built with -DDWBC_INST_MODEL"
#endif
#include <algorithm>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#ifndef EMU_IM_DYNAMICS_ONLY  // (the mutants: the dynamics kernel alone, seconds to compile)
#include "../../libdwbc_amd/csrc/dwbc_cycle2p.h"
#endif
#include "../../libdwbc_amd/csrc/dwbc_dynamics.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

namespace {
struct Ctx {
    Model m;
    Setup su;
    std::vector<int> topo;
};

int fail(char *err, int err_len, const std::string &s) {
    strncpy(err, s.c_str(), (size_t)err_len - 1);
    err[err_len - 1] = 0;
    return 0;
}

// the tree and the set-up tables of the model; its own mass, COM, inertia and joint frames are never handed to a kernel
bool make_ctx(Ctx &c, int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
              const double *inertia, std::string &e) {
    Model &m = c.m;
    m.parent.assign(parent, parent + nb);
    m.R_T.assign(R_T, R_T + 9 * nb);
    m.p_T.assign(p_T, p_T + 3 * nb);
    m.axis.assign(axis, axis + 3 * nb);
    m.mass.assign(mass, mass + nb);
    m.com.assign(com, com + 3 * nb);
    m.inertia.assign(inertia, inertia + 9 * nb);
    for (int i = 0; i < nb; i++) m.names.push_back("link" + std::to_string(i));
    m.finalize();
    setup_init(c.su, m.nb, m.ndof, m.maxdepth);
    m.topo_table(c.topo);
    setup_set_parents(c.su, c.topo.data());
    if (m.ndof != 39 || nb != 34 || c.su.topo_kind != 1) {
        e = "emu_inst_model: TOCABI's constant tree only";
        return false;
    }
    return true;
}

template <class F>
void each_instance(int B, size_t reals, F &&f) {
    std::vector<real_t> lds(reals + 64);
    for (int b = 0; b < B; b++) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<real_t>::quiet_NaN());
        f(b, lds.data());
    }
}
template <class F>
void with_levels(int n_levels, F &&f) {
    switch (n_levels) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{});
    }
}
}  // namespace

extern "C" {

#ifndef EMU_IM_DYNAMICS_ONLY
// build: 0 the extras build (Lds2), 1 the lean build on the compact map (Lds3), 2 the two-wave kernel (one and two levels), both roles in turn.
// contacts: n_contacts x [link, px py pz, lx ly mu muz] as doubles; tasks: per level and link slot [mode link px py pz] as doubles,
// t_nlinks[level] of kMaxTaskLinks slots used.  tables: B x nb x 25.  tau: B x 3 x 33, wrench: B x 12, status: B.
int emu_im_cycle(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                 const double *inertia, int n_contacts, const double *contacts, int n_levels, const int *t_nlinks, const double *tasks, const double *tau_lim,
                 int build, int hqp, int B, const double *tables, const double *q, const unsigned char *flags, const double *fstar, double *tau, double *wrench,
                 int *status, char *err, int err_len) {
    Ctx c;
    std::string e;
    if (!make_ctx(c, nb, parent, R_T, p_T, axis, mass, com, inertia, e)) return fail(err, err_len, e);
    for (int i = 0; i < n_contacts; i++) {
        const double *r = contacts + 8 * i;
        if (setup_add_contact(c.su, (int)r[0], 0, r + 1, r[4], r[5], r[6], r[7], e) < 0) return fail(err, err_len, e);
    }
    for (int l = 0; l < n_levels; l++)
        for (int j = 0; j < t_nlinks[l]; j++) {
            const double *r = tasks + 5 * (l * kMaxTaskLinks + j);
            if (!setup_add_task(c.su, l, (int)r[0], (int)r[1], r + 2, e)) return fail(err, err_len, e);
        }
    c.su.has_tau_lim = tau_lim != nullptr;
    for (int i = 0; tau_lim && i < c.m.ndof - 6; i++) c.su.tau_lim[i] = tau_lim[i];
    if (build == 2 && n_levels > 2) return fail(err, err_len, "the two-wave kernel is built for one and two task levels");
    std::vector<int> diag((size_t)B * DG_COUNT, -1);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar;
    io.tau = tau;
    io.wrench = wrench;
    io.status = status;
    io.diag = diag.data();
    io.body = tables;  // B tables back to back
    io.topo = c.topo.data();
    io.hqp = hqp;
    io.pair_swap_bit = -1;
    const Setup &su = c.su;
    const Thr th{0};
    std::vector<int> ilds(64);
    int *iL = ilds.data();
    with_levels(n_levels, [&](auto k) {
        constexpr int NLV = decltype(k)::value;
        if (build == 0)
            each_instance(B, Lds2<39, 34, 4>::total, [&](int b, real_t *L) { cycle_instance_v2<39, 34, NLV, 1, true, TopoTocabi>(th, su, io, b, L, iL); });
        else if (build == 1)
            each_instance(B, Lds2<39, 34, 4>::total, [&](int b, real_t *L) { cycle_instance_v2<39, 34, NLV, 1, false, TopoTocabi, true>(th, su, io, b, L, iL); });
        else if constexpr (NLV <= 2)
            each_instance(B, Lds4<39, 34, NLV>::total, [&](int b, real_t *L) { cycle_instance_v2p<39, 34, NLV, 1, TopoTocabi>(-1, th, su, io, b, L); });
    });
    return 1;
}

#endif

// q: B x 40; qd: B x 39 or NULL.  Every output of the dynamics kernel; tables as above.
int emu_im_dynamics(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                    const double *inertia, int B, const double *tables, const double *q, const double *qd, double *A, double *A_inv, double *Bv, double *G,
                    double *CMM, double *com_pos, int *status, char *err, int err_len) {
    Ctx c;
    std::string e;
    if (!make_ctx(c, nb, parent, R_T, p_T, axis, mass, com, inertia, e)) return fail(err, err_len, e);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.qdot = qd;
    io.body = tables;
    io.topo = c.topo.data();
    io.pair_swap_bit = -1;
    const DynIO dio{kDynA | kDynAInv | kDynB | kDynG | kDynCmm | kDynCom, A, A_inv, Bv, G, CMM, com_pos, status};
    each_instance(B, LdsDyn<39, 34>::total, [&](int b, real_t *L) { dynamics_instance<39, 34, 1, TopoTocabi>(Thr{0}, c.su, io, dio, b, L); });
    return 1;
}
}
