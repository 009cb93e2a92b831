// emu_task_space.cpp -- TEST HARNESS ONLY.  The task-space kernel source (libdwbc_amd/csrc/dwbc_task_space.h) compiled for the host with
// one "thread" per workgroup (NT = 1, barriers are no-ops): on TOCABI's constant tree, and on TopoGeneric at (37, 32) and TOCABI's (39, 34).
// A translation unit of its own: one entry point, the model given as arrays, one run described by its arguments.  LDS is exactly
// LdsTs<N, NB>::total doubles, NaN-poisoned before every instance, with a guard behind it that must come back untouched.  Loaded by
// tests/emu/emu_task_space.py.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_task_space.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

namespace {
constexpr int kGuard = 256;

template <int N, int NB, class Topo>
int run_size(const Setup &su, const BatchIO &io, const TsIO &tio, std::string &err) {
    const int total = LdsTs<N, NB>::total;
    std::vector<real_t> lds((size_t)total + kGuard);
    const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
    for (int b = 0; b < io.B; b++) {
        std::fill(lds.begin(), lds.begin() + total, nan);
        std::fill(lds.begin() + total, lds.end(), real_t(-7.0));
        task_space_instance<N, NB, 1, Topo>(Thr{0}, su, io, tio, b, lds.data());
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
int emu_task_space_lds_bytes(int n) {
    switch (n) {
    case 23: return LdsTs<23, 18>::total_bytes;
    case 37: return LdsTs<37, 32>::total_bytes;
    case 39: return LdsTs<39, 34>::total_bytes;
    case 43: return LdsTs<43, 38>::total_bytes;
    case 50: return LdsTs<50, 45>::total_bytes;  // the largest size a pack may have (the map only: the kernel is not instantiated here)
    }
    return 0;
}

// model: as emu_contact_space_run; nc registered contacts (link, point); nt task links in the order they are added, each (level, mode, link,
// point).  q: B x (ndof + 1); flags: B x nc.  mask: bits 1u << dwbc_task_space_output (the status is always written).  tree: 1 = TOCABI's
// constant tree (39 / 34 only), 0 = TopoGeneric.  out: 4 x kMaxLevels pointers, [what * 4 + level]; one that is not written may be NULL.
int emu_task_space_run(int nb, const int *parent, const double *R_T, const double *p_T, const double *axis, const double *mass, const double *com,
                       const double *inertia, int nc, const int *c_link, const double *c_point, int nt, const int *t_level, const int *t_mode,
                       const int *t_link, const double *t_point, int B, const double *q, const unsigned char *flags, unsigned mask, int tree,
                       double *const *out, int *status, char *err, int err_len) {
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
        if (setup_add_contact(su, c_link[i], 0, c_point + 3 * i, 0.15, 0.075, 0.2, 0.2, e) < 0) return fail(e);
    for (int i = 0; i < nt; i++)
        if (!setup_add_task(su, t_level[i], t_mode[i], t_link[i], t_point + 3 * i, e)) return fail(e);
    if (su.n_levels < 1 || setup_wide_tasks(su)) return fail("emu_task_space: 1 to 4 levels of at most 6 dof");
    BatchIO io{};  // the state, the flags and the model: every other pointer stays NULL, so a read of one faults here
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.body = body.data();
    io.topo = topo.data();
    io.hqp = 1;
    io.pair_swap_bit = -1;
    TsIO tio{};
    tio.mask = mask;
    for (int l = 0; l < kMaxLevels; l++) {
        tio.J_task[l] = out[0 * kMaxLevels + l];
        tio.Lambda[l] = out[1 * kMaxLevels + l];
        tio.J_kt[l] = out[2 * kMaxLevels + l];
        tio.Null[l] = out[3 * kMaxLevels + l];
    }
    tio.status = status;
    tio.cs_mask = ts_contact_stage_mask(mask);  // as dwbc_capi.hip launches it; cs_out stays NULL, so a store through it faults here
    if (tree) {
        if (m.ndof != 39 || nb != 34 || su.topo_kind != 1) return fail("emu_task_space: the constant tree is TOCABI's");
        return run_size<39, 34, TopoTocabi>(su, io, tio, e) ? 1 : fail(e);
    }
    if (m.ndof == 37 && nb == 32) return run_size<37, 32, TopoGeneric>(su, io, tio, e) ? 1 : fail(e);
    if (m.ndof == 39 && nb == 34) return run_size<39, 34, TopoGeneric>(su, io, tio, e) ? 1 : fail(e);
    return fail("emu_task_space is instantiated for (37, 32) and (39, 34)");
}
}
