// emu_redist_sizes.cpp -- TEST HARNESS ONLY.  The redistribution kernel source (libdwbc_amd/csrc/dwbc_redistribute.h) compiled for the host
// with one "thread" per workgroup (NT = 1, barriers are no-ops) at the sizes the kernel packs are built for, on TopoGeneric: (23, 18),
// (37, 32), (43, 38) and TOCABI's (39, 34).  emu_cycle.cpp runs the kernel on TOCABI's constant tree alone; here the arithmetic and the
// indexing of the text that ships are checked at the other sizes against the numpy restatement without a GPU.  A translation unit of its
// own: one entry point, the model given as arrays, one run described by its arguments.  LDS is exactly LdsRd<N, NB>::total doubles,
// NaN-poisoned before every instance, with a guard behind it that must come back untouched.  Loaded by tests/emu/emu_redist_sizes.py.
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

template <int N, int NB>
int run_size(const Setup &su, const BatchIO &io, const RedistIO &rio, std::string &err) {
    const int total = LdsRd<N, NB>::total;
    std::vector<real_t> lds((size_t)total + kGuard);
    const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
    for (int b = 0; b < io.B; b++) {
        std::fill(lds.begin(), lds.begin() + total, nan);
        std::fill(lds.begin() + total, lds.end(), real_t(-7.0));
        redistribute_instance<N, NB, 1, TopoGeneric>(Thr{0}, su, io, rio, b, lds.data());
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

// total_bytes of the map at one of the instantiated sizes; 0: not instantiated
int emu_redist_sizes_lds_bytes(int n) {
    switch (n) {
    case 23: return LdsRd<23, 18>::total_bytes;
    case 37: return LdsRd<37, 32>::total_bytes;
    case 39: return LdsRd<39, 34>::total_bytes;
    case 43: return LdsRd<43, 38>::total_bytes;
    case 50: return LdsRd<50, 45>::total_bytes;  // the largest size a pack may have (the map only: the kernel is not instantiated here)
    }
    return 0;
}

// model: nb bodies as arrays (parent, R_T nb x 9, p_T nb x 3, axis nb x 3, mass nb, com nb x 3, inertia nb x 9).  contacts: nc x (link),
// nc x 3 points, nc x 4 (lx, ly, mu, muz).  tau_lim: nb - 1 or NULL.  q: B x (ndof + 1), flags: B x nc, tau_in: B x (ndof - 6),
// inst_par: B x (ndof - 6 + 4 nc) or NULL.  Outputs: tau B x (ndof - 6), cf B x 6, wrench B x 24, status B.  Returns 1, or 0 with err.
int emu_redist_sizes_run(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                         const double *inertia, int nc, const int *c_link, const double *c_point, const double *c_par, const double *tau_lim, int B,
                         const double *q, const unsigned char *flags, const double *tau_in, const double *inst_par, double *tau, double *cf, double *wrench,
                         int *status, char *err, int err_len) {
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
    const RedistIO rio{tau_in, tau, cf, wrench, status};
    if (m.ndof == 23 && nb == 18) return run_size<23, 18>(su, io, rio, e) ? 1 : fail(e);
    if (m.ndof == 37 && nb == 32) return run_size<37, 32>(su, io, rio, e) ? 1 : fail(e);
    if (m.ndof == 39 && nb == 34) return run_size<39, 34>(su, io, rio, e) ? 1 : fail(e);
    if (m.ndof == 43 && nb == 38) return run_size<43, 38>(su, io, rio, e) ? 1 : fail(e);
    return fail("emu_redist_sizes is instantiated for (23, 18), (37, 32), (39, 34) and (43, 38)");
}
}
