// emu_inst_par.cpp -- TEST HARNESS ONLY.  Host build of the one-wave cycle (libdwbc_amd/csrc/dwbc_cycle2.h) and of the redistribution
// kernel (dwbc_redistribute.h) with one "thread" per workgroup, as emu_cycle.cpp / emu_redist.cpp, run with a per-instance parameter
// record (BatchIO::inst_par) or without one: the record's indexing and the row constants it replaces are checked against the restatement
// without a GPU.  LDS is NaN-poisoned before every instance.  As the launcher does (dwbc_capi.hip: launch_setup), a run with a record
// hands the kernel a set-up whose torque rows exist.  Never linked into libdwbc_hip.so.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_redistribute.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

struct IpCtx {
    Model model;
    Setup su;
    std::vector<double> body;
    std::vector<int> topo;
    std::string err;
};

static Setup with_record(const Setup &su, const double *inst_par) {
    Setup s = su;
    if (inst_par) s.has_tau_lim = 1;
    return s;
}

extern "C" {

IpCtx *ip_create(const char *urdf) {
    auto *c = new IpCtx();
    if (!load_urdf(urdf, true, c->model, c->err)) return c;
    setup_init(c->su, c->model.nb, c->model.ndof, c->model.maxdepth);
    c->model.body_table(c->body);
    c->model.topo_table(c->topo);
    setup_set_parents(c->su, c->topo.data());
    return c;
}
const char *ip_error(IpCtx *c) { return c->err.c_str(); }
void ip_destroy(IpCtx *c) { delete c; }
int ip_ndof(IpCtx *c) { return c->model.ndof; }
int ip_add_contact(IpCtx *c, int link, const double *pt, double lx, double ly, double mu, double muz) {
    return setup_add_contact(c->su, link, 0, pt, lx, ly, mu, muz, c->err);
}
int ip_add_task(IpCtx *c, int level, int mode, int link, const double *pt) { return setup_add_task(c->su, level, mode, link, pt, c->err) ? 1 : 0; }
int ip_fstar_total(IpCtx *c) { return c->su.fstar_total; }
void ip_set_tau_lim(IpCtx *c, const double *lim) {
    c->su.has_tau_lim = lim != nullptr;
    if (lim) for (int i = 0; i < c->model.ndof - 6; i++) c->su.tau_lim[i] = lim[i];
}
int ip_stride(IpCtx *c) { return c->model.ndof - 6 + 4 * c->su.n_contacts; }

// the one-wave cycle for two task levels: compact = 1 the lean build on the compact map (Lds3), 0 the extras build (Lds2)
int ip_run_cycle(IpCtx *c, int B, const double *q, const unsigned char *flags, const double *fstar, const double *inst_par, int compact, double *tau,
                 double *wrench, int *status, int *diag) {
    if (c->model.ndof != 39 || c->model.nb != 34 || c->su.n_levels != 2) { c->err = "emu is instantiated for TOCABI (39 dof), two task levels"; return 0; }
    const Setup su = with_record(c->su, inst_par);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar;
    io.tau = tau;
    io.wrench = wrench;
    io.status = status;
    io.diag = diag;
    io.body = c->body.data();
    io.topo = c->topo.data();
    io.hqp = 1;
    io.pair_swap_bit = -1;
    io.inst_par = inst_par;
    std::vector<real_t> lds(Lds2<39, 34, 2>::total + 64);
    std::vector<int> ilds(64);
    for (int b = 0; b < B; b++) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<real_t>::quiet_NaN());
        if (compact) cycle_instance_v2<39, 34, 2, 1, false, TopoTocabi, true>(Thr{0}, su, io, b, lds.data(), ilds.data());
        else cycle_instance_v2<39, 34, 2, 1, true, TopoTocabi>(Thr{0}, su, io, b, lds.data(), ilds.data());
    }
    return 1;
}

int ip_run_redist(IpCtx *c, int B, const double *q, const unsigned char *flags, const double *fstar, const double *tau_in, const double *inst_par,
                  double *tau, double *cf, double *wrench, int *status) {
    if (c->model.ndof != 39 || c->model.nb != 34) { c->err = "emu is instantiated for TOCABI (39 dof) only"; return 0; }
    const Setup su = with_record(c->su, inst_par);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar;
    io.body = c->body.data();
    io.topo = c->topo.data();
    io.hqp = 1;
    io.inst_par = inst_par;
    RedistIO rio{tau_in, tau, cf, wrench, status};
    std::vector<real_t> lds(LdsRd<39, 34>::total + 8);
    for (int b = 0; b < B; b++) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<real_t>::quiet_NaN());
        redistribute_instance<39, 34, 1, TopoTocabi>(Thr{0}, su, io, rio, b, lds.data());
    }
    return 1;
}
}
