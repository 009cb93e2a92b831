// emu_redist.cpp -- TEST HARNESS ONLY.  Host build of the redistribution kernel's source (libdwbc_amd/csrc/dwbc_redistribute.h) with one
// "thread" per workgroup, as emu_cycle.cpp does for the cycle kernels: the arithmetic, the indexing and the LDS life times (LDS is
// NaN-poisoned before every instance) are checked against the restatement without a GPU.  Never linked into libdwbc_hip.so.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_redistribute.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"
#include "../../libdwbc_amd/csrc/dwbc_setup.h"

using namespace dwbc;

struct RdCtx {
    Model model;
    Setup su;
    std::vector<double> body;
    std::vector<int> topo;
    std::string err;
};

extern "C" {

RdCtx *rd_create(const char *urdf) {
    auto *c = new RdCtx();
    if (!load_urdf(urdf, true, c->model, c->err)) return c;
    setup_init(c->su, c->model.nb, c->model.ndof, c->model.maxdepth);
    c->model.body_table(c->body);
    c->model.topo_table(c->topo);
    setup_set_parents(c->su, c->topo.data());
    return c;
}
const char *rd_error(RdCtx *c) { return c->err.c_str(); }
void rd_destroy(RdCtx *c) { delete c; }
int rd_ndof(RdCtx *c) { return c->model.ndof; }
int rd_add_contact(RdCtx *c, int link, const double *pt, double lx, double ly, double mu, double muz) {
    return setup_add_contact(c->su, link, 0, pt, lx, ly, mu, muz, c->err);
}
// task levels play no part in the redistribution; a set-up that has some (the facade's, a cycle batch's) must give the same answer
int rd_add_task(RdCtx *c, int level, int mode, int link, const double *pt) { return setup_add_task(c->su, level, mode, link, pt, c->err) ? 1 : 0; }
int rd_fstar_total(RdCtx *c) { return c->su.fstar_total; }
void rd_set_tau_lim(RdCtx *c, const double *lim) {
    c->su.has_tau_lim = lim != nullptr;
    if (lim) for (int i = 0; i < c->model.ndof - 6; i++) c->su.tau_lim[i] = lim[i];
}
int rd_lds_bytes() { return LdsRd<39, 34>::total_bytes; }

int rd_run(RdCtx *c, int B, const double *q, const unsigned char *flags, const double *fstar, const double *tau_in, double *tau, double *cf,
           double *wrench, int *status) {
    if (c->model.ndof != 39 || c->model.nb != 34) { c->err = "emu is instantiated for TOCABI (39 dof) only"; return 0; }
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.flags = flags;
    io.fstar = fstar;
    io.body = c->body.data();
    io.topo = c->topo.data();
    io.hqp = 1;
    RedistIO rio{tau_in, tau, cf, wrench, status};
    std::vector<real_t> lds(LdsRd<39, 34>::total + 8);
    for (int b = 0; b < B; b++) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<real_t>::quiet_NaN());
        redistribute_instance<39, 34, 1, TopoTocabi>(Thr{0}, c->su, io, rio, b, lds.data());
    }
    return 1;
}
}
