// emu_gravcomp.cpp -- TEST HARNESS ONLY.  The gravity-compensation build of the redistribution kernel source
// (libdwbc_amd/csrc/dwbc_redistribute.h, GRAV = true) compiled for the host with one "thread" per workgroup (NT = 1, barriers are no-ops):
// on TopoGeneric at (23, 18), (37, 32), (43, 38) and TOCABI's (39, 34), and on TOCABI's constant tree.  Both forms of the launch: gravity
// only (tau_in = NULL) and the redistribution of torque_grav_ + tau_in.  A translation unit of its own: one entry point, the model given as
// arrays, one run described by its arguments.  LDS is exactly LdsGc<N, NB>::total doubles, NaN-poisoned before every instance, with a
// guard behind it that must come back untouched.  Loaded by tests/emu/emu_gravcomp.py.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_redistribute.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

namespace {
constexpr int kGuard = 256;

template <int N, int NB, class Topo>
int run_size(const Setup &su, const BatchIO &io, const GravIO &gio, std::string &err) {
    const int total = LdsGc<N, NB>::total;
    std::vector<real_t> lds((size_t)total + kGuard);
    const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
    const RedistIO rio{gio.tau_in, gio.rd_tau, gio.rd_cf, gio.rd_wrench, gio.rd_status};
    for (int b = 0; b < io.B; b++) {
        std::fill(lds.begin(), lds.begin() + total, nan);
        std::fill(lds.begin() + total, lds.end(), real_t(-7.0));
        redistribute_instance<N, NB, 1, Topo, true>(Thr{0}, su, io, rio, b, lds.data(), &gio);
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
int emu_gravcomp_lds_bytes(int n) {
    switch (n) {
    case 23: return LdsGc<23, 18>::total_bytes;
    case 37: return LdsGc<37, 32>::total_bytes;
    case 39: return LdsGc<39, 34>::total_bytes;
    case 43: return LdsGc<43, 38>::total_bytes;
    case 50: return LdsGc<50, 45>::total_bytes;  // the largest size a pack may have (the map only: the kernel is not instantiated here)
    }
    return 0;
}

// model, contacts, tau_lim, q, flags, inst_par: as emu_redist_sizes_run.  tau_in: B x (ndof - 6), or NULL for the gravity-only form (the
// four rd_* outputs are then not touched).  tree: 1 = TOCABI's constant tree (39 / 34 only), 0 = TopoGeneric.
// Outputs: rd_tau B x (ndof - 6), rd_cf B x 6, rd_wrench B x 24, rd_status B; g_tau B x (ndof - 6), g_wrench B x 12, g_status B.
int emu_gravcomp_run(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                     const double *inertia, int nc, const int *c_link, const double *c_point, const double *c_par, const double *tau_lim, int B,
                     const double *q, const unsigned char *flags, const double *tau_in, const double *inst_par, int tree, double *rd_tau, double *rd_cf,
                     double *rd_wrench, int *rd_status, double *g_tau, double *g_wrench, int *g_status, char *err, int err_len) {
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
    su.has_tau_lim = tau_lim != nullptr || inst_par != nullptr;  // (as the launcher: a per-instance record brings torque rows of its own)
    if (tau_lim)
        for (int i = 0; i < m.ndof - 6; i++) su.tau_lim[i] = tau_lim[i];
    std::vector<double> fstar((size_t)B, 0.0);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar.data();
    io.body = body.data();
    io.topo = topo.data();
    io.hqp = 1;
    io.pair_swap_bit = -1;
    io.inst_par = inst_par;
    const GravIO gio{tau_in, rd_tau, rd_cf, rd_wrench, rd_status, g_tau, g_wrench, g_status};
    if (tree) {
        if (m.ndof != 39 || nb != 34 || su.topo_kind != 1) return fail("emu_gravcomp: the constant tree is TOCABI's");
        return run_size<39, 34, TopoTocabi>(su, io, gio, e) ? 1 : fail(e);
    }
    if (m.ndof == 23 && nb == 18) return run_size<23, 18, TopoGeneric>(su, io, gio, e) ? 1 : fail(e);
    if (m.ndof == 37 && nb == 32) return run_size<37, 32, TopoGeneric>(su, io, gio, e) ? 1 : fail(e);
    if (m.ndof == 39 && nb == 34) return run_size<39, 34, TopoGeneric>(su, io, gio, e) ? 1 : fail(e);
    if (m.ndof == 43 && nb == 38) return run_size<43, 38, TopoGeneric>(su, io, gio, e) ? 1 : fail(e);
    return fail("emu_gravcomp is instantiated for (23, 18), (37, 32), (39, 34) and (43, 38)");
}
}
