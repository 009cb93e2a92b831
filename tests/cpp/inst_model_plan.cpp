// inst_model_plan.cpp -- dwbc_plan::plan() (libdwbc_amd/csrc/dwbc_launch_plan.h) for a batch that carries one body table per instance
// (Request::inst_model), over a hand-written table: TOCABI's rows in both arithmetic types with the rows of the six lean launches, the rows
// of the per-instance-model build (namespace dwbc_im, flavour bit kInstModel: the 18 cycle kernels and the six lean launches on TOCABI's
// tree) as a table of their own, and a 37-dof / 32-body pack.  No GPU, no HIP.  Every argument is one request, `key=value,key=value` over
// the defaults below (`im_table=0` leaves the dwbc_im table out); the answer to each is one JSON line.  Driven by
// tests/test_instance_model_plan.py.
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_launch_plan.h"

using namespace dwbc_plan;

static std::deque<std::string> g_strings;
static char g_kernels[512];
static int g_n_kernels = 0;

static Row row(int n, int nb, int nlv, int topo, int arith, int kind, unsigned flavour, int lds, int threads, const std::string &base, const std::string &tail) {
    g_strings.push_back(base);
    const char *b = g_strings.back().c_str();
    g_strings.push_back(tail);
    return Row{n, nb, nlv, topo, arith, kind, flavour, &g_kernels[g_n_kernels++], lds, threads, b, g_strings.back().c_str()};
}

// im: the per-instance-model build -- the namespace is dwbc_im, every row carries kInstModel, and only what that build instantiates is listed
static std::vector<Row> tocabi(int arith, bool im) {
    const std::string ns = im ? "dwbc_im::" : arith == kFloat ? "dwbc_f32::" : "dwbc::";
    const unsigned x = im ? (unsigned)kInstModel : 0u;
    std::vector<Row> t;
    for (int lv = 1; lv <= 4; lv++) {
        const std::string s = "39, 34, " + std::to_string(lv);
        if (!im) {
            t.push_back(row(39, 34, lv, 0, arith, kCycle, 0, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, true, " + ns + "TopoGeneric"));
            t.push_back(row(39, 34, lv, 0, arith, kReduced, 0, 50000 + lv, 64, ns + "dwbc_cycle_kernel_reduced", s + ", 64, " + ns + "TopoGeneric"));
            t.push_back(row(39, 34, lv, 1, arith, kReduced, 0, 50000 + lv, 64, ns + "dwbc_cycle_kernel_reduced", s + ", 64, " + ns + "TopoTocabi"));
        }
        t.push_back(row(39, 34, lv, 1, arith, kCycle, x, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, true, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, x | kWide, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2w", s + ", 64, true, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, x | kWide | kLean, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2w", s + ", 64, false, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, x | kLean | kCompact, 20000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, false, " + ns + "TopoTocabi, true"));
        if (arith == kDouble && lv <= 2)
            t.push_back(row(39, 34, lv, 1, arith, kCycle, x | kLean | kTwoWave, 40000 + lv, 128, ns + "dwbc_cycle_kernel_v2p", s + ", " + ns + "TopoTocabi"));
    }
    if (arith == kDouble) {
        if (!im) {
            t.push_back(row(39, 34, 0, 0, arith, kGc, 0, 81696, 64, ns + "dwbc_cycle_kernel_gc", "39, 34, 64, 6"));
            t.push_back(row(39, 34, 0, 0, arith, kGc, kWideTasks, 105000, 64, ns + "dwbc_cycle_kernel_gc", "39, 34, 64, 12"));
        }
        const char *lean[][2] = {{"dwbc_redistribute_kernel", nullptr}, {"dwbc_gravcomp_kernel", nullptr}, {"dwbc_dynamics_kernel", nullptr},
                                 {"dwbc_contact_space_kernel", nullptr}, {"dwbc_task_space_kernel", nullptr}};
        const int kinds[] = {kRedist, kGravComp, kDynamics, kContactSpace, kTaskSpace};
        for (int i = 0; i < 5; i++) {
            t.push_back(row(39, 34, 0, 1, arith, kinds[i], x, 20000 + i, 64, ns + lean[i][0], "39, 34, " + ns + "TopoTocabi"));
            if (!im) t.push_back(row(39, 34, 0, 0, arith, kinds[i], 0, 20000 + i, 64, ns + lean[i][0], "39, 34, " + ns + "TopoGeneric"));
        }
        t.push_back(row(39, 34, 0, 0, arith, kLinkQuery, x, 13000, 64, ns + "dwbc_link_query_kernel", "39, 34"));
    }
    return t;
}

static std::vector<Row> pack_37_32() {
    std::vector<Row> t;
    for (int lv = 1; lv <= 4; lv++) {
        const std::string s = "37, 32, " + std::to_string(lv);
        t.push_back(row(37, 32, lv, 0, kDouble, kCycle, 0, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2", s + ", 64, true, dwbc::TopoGeneric"));
        t.push_back(row(37, 32, lv, 0, kDouble, kCycle, kWide | kLean, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2w", s + ", 64, false, dwbc::TopoGeneric"));
    }
    t.push_back(row(37, 32, 0, 0, kDouble, kDynamics, 0, 14000, 64, "dwbc::dwbc_dynamics_kernel", "37, 32, dwbc::TopoGeneric"));
    return t;
}

static bool g_im_table = true;

static Request parse(const char *arg) {
    Request q{};
    q.n = 39, q.nb = 34, q.levels = 2, q.topo = 1, q.arith = kDouble, q.B = 250, q.n_cu = 256, q.max_active = 2, q.hqp = true, q.pair_swap_bit = -1;
    q.n_contacts = 2;
    g_im_table = true;
    std::string s(arg);
    for (size_t a = 0; a < s.size();) {
        size_t e = s.find(',', a);
        if (e == std::string::npos) e = s.size();
        const std::string kv = s.substr(a, e - a), k = kv.substr(0, kv.find('='));
        const int v = atoi(kv.c_str() + kv.find('=') + 1);
        a = e + 1;
        if (k == "n") q.n = v;
        else if (k == "nb") q.nb = v;
        else if (k == "levels") q.levels = v;
        else if (k == "topo") q.topo = v;
        else if (k == "arith") q.arith = v;
        else if (k == "B") q.B = v;
        else if (k == "n_cu") q.n_cu = v;
        else if (k == "reduced") q.reduced = v;
        else if (k == "max_active") q.max_active = v;
        else if (k == "wide_tasks") q.wide_tasks = v;
        else if (k == "hqp") q.hqp = v;
        else if (k == "warm") q.warm = v;
        else if (k == "n_traj") q.n_traj = v;
        else if (k == "has_com_task") q.has_com_task = v;
        else if (k == "n_custom") q.n_custom = v;
        else if (k == "dump_on") q.dump_on = v;
        else if (k == "no_wide") q.no_wide = v;
        else if (k == "no_pair") q.no_pair = v;
        else if (k == "no_lean") q.no_lean = v;
        else if (k == "pair_always") q.pair_always = v;
        else if (k == "pair_swap_bit") q.pair_swap_bit = v;
        else if (k == "redistribute") q.redistribute = v;
        else if (k == "grav_comp") q.grav_comp = v;
        else if (k == "link_query") q.link_query = v;
        else if (k == "dynamics") q.dynamics = v;
        else if (k == "contact_space") q.contact_space = v;
        else if (k == "task_space") q.task_space = v;
        else if (k == "n_contacts") q.n_contacts = v;
        else if (k == "inst_par") q.inst_par = v;
        else if (k == "inst_model") q.inst_model = v;
        else if (k == "im_table") g_im_table = v;
        else if (!kv.empty()) {
            fprintf(stderr, "unknown key '%s'\n", k.c_str());
            exit(2);
        }
    }
    return q;
}

int main(int argc, char **argv) {
    const std::vector<Row> f64 = tocabi(kDouble, false), f32 = tocabi(kFloat, false), im = tocabi(kDouble, true), pack = pack_37_32();
    const Table with_im[4] = {{f64.data(), (int)f64.size()}, {f32.data(), (int)f32.size()}, {im.data(), (int)im.size()}, {pack.data(), (int)pack.size()}};
    const Table without[3] = {with_im[0], with_im[1], with_im[3]};
    for (int i = 1; i < argc; i++) {
        const Request q = parse(argv[i]);
        const Plan p = g_im_table ? plan(q, with_im, 4) : plan(q, without, 3);
        char name[160] = "";
        if (p.row) format_name(*p.row, name, sizeof name);
        printf("{\"name\": \"%s\", \"threads\": %d, \"lds\": %d, \"ws_valid_after\": %s, \"pair_swap_bit\": %d, \"flavour\": %u, \"err\": \"%s\"}\n", name, p.threads,
               p.lds, p.ws_valid_after ? "true" : "false", p.pair_swap_bit, p.row ? p.row->flavour : 0u, p.err ? p.err : "");
    }
    return 0;
}
