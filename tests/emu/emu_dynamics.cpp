// emu_dynamics.cpp -- TEST HARNESS ONLY.  The dynamics kernel source (libdwbc_amd/csrc/dwbc_dynamics.h) compiled for the host with one
// "thread" per workgroup (NT = 1, barriers are no-ops): on TOCABI's constant tree, and on TopoGeneric at (23, 18), (37, 32), (43, 38) and
// TOCABI's (39, 34).  A translation unit of its own: one entry point, the model given as arrays, one run described by its arguments.  LDS
// is exactly LdsDyn<N, NB>::total doubles, NaN-poisoned before every instance, with a guard behind it that must come back untouched.
// Loaded by tests/emu/emu_dynamics.py.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_dynamics.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

namespace {
constexpr int kGuard = 256;

template <int N, int NB, class Topo>
int run_size(const Setup &su, const BatchIO &io, const DynIO &dio, std::string &err) {
    const int total = LdsDyn<N, NB>::total;
    std::vector<real_t> lds((size_t)total + kGuard);
    const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
    for (int b = 0; b < io.B; b++) {
        std::fill(lds.begin(), lds.begin() + total, nan);
        std::fill(lds.begin() + total, lds.end(), real_t(-7.0));
        dynamics_instance<N, NB, 1, Topo>(Thr{0}, su, io, dio, b, lds.data());
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
int emu_dynamics_lds_bytes(int n) {
    switch (n) {
    case 23: return LdsDyn<23, 18>::total_bytes;
    case 37: return LdsDyn<37, 32>::total_bytes;
    case 39: return LdsDyn<39, 34>::total_bytes;
    case 43: return LdsDyn<43, 38>::total_bytes;
    case 50: return LdsDyn<50, 45>::total_bytes;  // the largest size a pack may have (the map only: the kernel is not instantiated here)
    }
    return 0;
}

// model: as emu_gravcomp_run.  q: B x (ndof + 1); qd: B x ndof or NULL.  mask: bits 1u << dwbc_dynamics_output (the status is always
// written).  tree: 1 = TOCABI's constant tree (39 / 34 only), 0 = TopoGeneric.  An output whose bit is clear may be NULL.
int emu_dynamics_run(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                     const double *inertia, int B, const double *q, const double *qd, unsigned mask, int tree, double *A, double *A_inv, double *Bv,
                     double *G, double *CMM, double *com_pos, int *status, char *err, int err_len) {
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
    BatchIO io{};  // the state and the model: every other pointer stays NULL, so a read of one faults here
    io.B = B;
    io.q = q;
    io.qdot = qd;
    io.body = body.data();
    io.topo = topo.data();
    io.pair_swap_bit = -1;
    const DynIO dio{mask, A, A_inv, Bv, G, CMM, com_pos, status};
    std::string e;
    if (tree) {
        if (m.ndof != 39 || nb != 34 || su.topo_kind != 1) return fail("emu_dynamics: the constant tree is TOCABI's");
        return run_size<39, 34, TopoTocabi>(su, io, dio, e) ? 1 : fail(e);
    }
    if (m.ndof == 23 && nb == 18) return run_size<23, 18, TopoGeneric>(su, io, dio, e) ? 1 : fail(e);
    if (m.ndof == 37 && nb == 32) return run_size<37, 32, TopoGeneric>(su, io, dio, e) ? 1 : fail(e);
    if (m.ndof == 39 && nb == 34) return run_size<39, 34, TopoGeneric>(su, io, dio, e) ? 1 : fail(e);
    if (m.ndof == 43 && nb == 38) return run_size<43, 38, TopoGeneric>(su, io, dio, e) ? 1 : fail(e);
    return fail("emu_dynamics is instantiated for (23, 18), (37, 32), (39, 34) and (43, 38)");
}
}
