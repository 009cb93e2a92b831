// emu_link_query.cpp -- TEST HARNESS ONLY.  The link-query kernel source (libdwbc_amd/csrc/dwbc_link_query.h) compiled for the host with one
// "thread" per workgroup (NT = 1, barriers are no-ops), as emu_cycle.cpp does for the cycle kernels: the arithmetic and the indexing of
// the text that ships are checked against the numpy restatement without a GPU.  A translation unit of its own (the kernel needs nothing
// of the cycle's harness): one entry point, one run described by its arguments, LDS poisoned with NaN before every instance.  Loaded by
// tests/emu/emu_link_query.py.
#define DWBC_HOST_EMU 1
#include <algorithm>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_link_query.h"
#include "../../libdwbc_amd/csrc/dwbc_model.h"

using namespace dwbc;

extern "C" {

int emu_link_query_lds_bytes() { return LdsLq<39, 34>::total_bytes; }
int emu_link_query_max_entries() { return kMaxLinkQuery; }

// q: B x 40, qdot: B x 39 or NULL, links: n, points: n x 3; pos B x n x 3, rot B x n x 9, vel B x n x 6, jac B x n x 6 x 39 or NULL.
// Returns 1, or 0 with a message in err.
int emu_link_query_run(const char *urdf, int B, const double *q, const double *qdot, int n, const int *links, const double *points, double *pos,
                       double *rot, double *vel, double *jac, char *err, int err_len) {
    auto fail = [&](const std::string &s) {
        strncpy(err, s.c_str(), (size_t)err_len - 1);
        err[err_len - 1] = 0;
        return 0;
    };
    Model m;
    std::string e;
    if (!load_urdf(urdf, true, m, e)) return fail(e);
    if (m.ndof != 39 || m.nb != 34) return fail("emu_link_query is instantiated for 39 dof / 34 bodies");
    if (n < 1 || n > kMaxLinkQuery) return fail("1 .. 16 entries");
    std::vector<double> body;
    std::vector<int> topo;
    m.body_table(body);
    m.topo_table(topo);
    BatchIO io{};
    io.B = B;
    io.q = q;
    io.qdot = qdot;
    io.body = body.data();
    io.topo = topo.data();
    LinkQueryIO lq{};
    lq.n = n;
    lq.nb = m.nb;
    lq.maxdepth = m.maxdepth;
    lq.want_jac = jac != nullptr;
    for (int i = 0; i < n; i++) {
        if (links[i] < 0 || links[i] > m.nb) return fail("link out of range");
        lq.link[i] = links[i];
        lq.has_com = lq.has_com || links[i] == m.nb;
        for (int a = 0; a < 3; a++) lq.point[i][a] = points[i * 3 + a];
    }
    lq.pos = pos;
    lq.rot = rot;
    lq.vel = vel;
    lq.jac = jac;
    std::vector<real_t> lds(LdsLq<39, 34>::total + 64);
    for (int b = 0; b < B; b++) {
        std::fill(lds.begin(), lds.end(), std::numeric_limits<real_t>::quiet_NaN());
        link_query_instance<39, 34, 1>(Thr{0}, io, lq, b, lds.data());
    }
    return 1;
}
}
