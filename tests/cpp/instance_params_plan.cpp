// instance_params_plan.cpp -- dwbc_plan::plan() (libdwbc_amd/csrc/dwbc_launch_plan.h) for a batch that carries per-instance torque limits
// and contact cone constants (Request::inst_par), over a hand-written table: TOCABI's rows in both arithmetic types with the redistribution
// row, and a 37-dof / 32-body pack in its generic and its tree-specific build.  No GPU, no HIP.  Every argument is one request,
// `key=value,key=value` over the defaults below; the answer to each is one JSON line.  Driven by tests/test_instance_params_plan.py.
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_launch_plan.h"

using namespace dwbc_plan;

static std::deque<std::string> g_strings;
static char g_kernels[256];
static int g_n_kernels = 0;

static Row row(int n, int nb, int nlv, int topo, int arith, int kind, unsigned flavour, int lds, int threads, const std::string &base, const std::string &tail) {
    g_strings.push_back(base);
    const char *b = g_strings.back().c_str();
    g_strings.push_back(tail);
    return Row{n, nb, nlv, topo, arith, kind, flavour, &g_kernels[g_n_kernels++], lds, threads, b, g_strings.back().c_str()};
}

// four level counts x (capped extras, wide extras, wide lean, compact lean, any-tree capped extras) + reduced on both trees; fp64 adds
// the two-wave kernel for one and two levels and the two general-contact kernels
static std::vector<Row> tocabi(int arith) {
    const std::string ns = arith == kFloat ? "dwbc_f32::" : "dwbc::";
    std::vector<Row> t;
    for (int lv = 1; lv <= 4; lv++) {
        const std::string s = "39, 34, " + std::to_string(lv);
        // (the any-tree rows first: the planner must prefer the tree's own whatever the order)
        t.push_back(row(39, 34, lv, 0, arith, kCycle, 0, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, true, " + ns + "TopoGeneric"));
        t.push_back(row(39, 34, lv, 0, arith, kReduced, 0, 50000 + lv, 64, ns + "dwbc_cycle_kernel_reduced", s + ", 64, " + ns + "TopoGeneric"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, 0, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, true, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, kWide, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2w", s + ", 64, true, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, kWide | kLean, 31000 + lv, 64, ns + "dwbc_cycle_kernel_v2w", s + ", 64, false, " + ns + "TopoTocabi"));
        t.push_back(row(39, 34, lv, 1, arith, kCycle, kLean | kCompact, 20000 + lv, 64, ns + "dwbc_cycle_kernel_v2", s + ", 64, false, " + ns + "TopoTocabi, true"));
        t.push_back(row(39, 34, lv, 1, arith, kReduced, 0, 50000 + lv, 64, ns + "dwbc_cycle_kernel_reduced", s + ", 64, " + ns + "TopoTocabi"));
        if (arith == kDouble && lv <= 2)
            t.push_back(row(39, 34, lv, 1, arith, kCycle, kLean | kTwoWave, 40000 + lv, 128, ns + "dwbc_cycle_kernel_v2p", s + ", " + ns + "TopoTocabi"));
    }
    if (arith == kDouble) {
        t.push_back(row(39, 34, 0, 0, arith, kGc, 0, 81696, 64, ns + "dwbc_cycle_kernel_gc", "39, 34, 64, 6"));
        t.push_back(row(39, 34, 0, 0, arith, kGc, kWideTasks, 105000, 64, ns + "dwbc_cycle_kernel_gc", "39, 34, 64, 12"));
        t.push_back(row(39, 34, 0, 1, arith, kRedist, 0, 20432, 64, ns + "dwbc_redistribute_kernel", "39, 34, " + ns + "TopoTocabi"));
    }
    return t;
}

static std::vector<Row> pack_37_32(int topo) {
    const std::string tp = topo == 2 ? "dwbc::TopoPack" : "dwbc::TopoGeneric";
    std::vector<Row> t;
    for (int lv = 1; lv <= 4; lv++) {
        const std::string s = "37, 32, " + std::to_string(lv);
        t.push_back(row(37, 32, lv, topo, kDouble, kCycle, 0, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2", s + ", 64, true, " + tp));
        t.push_back(row(37, 32, lv, topo, kDouble, kCycle, kWide, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2w", s + ", 64, true, " + tp));
        t.push_back(row(37, 32, lv, topo, kDouble, kCycle, kLean, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2", s + ", 64, false, " + tp));
        t.push_back(row(37, 32, lv, topo, kDouble, kCycle, kWide | kLean, 29000 + lv, 64, "dwbc::dwbc_cycle_kernel_v2w", s + ", 64, false, " + tp));
    }
    t.push_back(row(37, 32, 0, 0, kDouble, kGc, 0, 78000, 64, "dwbc::dwbc_cycle_kernel_gc", "37, 32, 64, 6"));
    return t;
}

static Request parse(const char *arg) {
    Request q{};
    q.n = 39, q.nb = 34, q.levels = 2, q.topo = 1, q.arith = kDouble, q.B = 250, q.n_cu = 256, q.max_active = 2, q.hqp = true, q.pair_swap_bit = -1;
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
        else if (k == "tree_match") q.tree_match = v;
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
        else if (k == "inst_par") q.inst_par = v;
        else if (!kv.empty()) {
            fprintf(stderr, "unknown key '%s'\n", k.c_str());
            exit(2);
        }
    }
    return q;
}

int main(int argc, char **argv) {
    const std::vector<Row> f64 = tocabi(kDouble), f32 = tocabi(kFloat), tree = pack_37_32(2), generic = pack_37_32(0);
    const Table tabs[4] = {{f64.data(), (int)f64.size()}, {f32.data(), (int)f32.size()}, {tree.data(), (int)tree.size()}, {generic.data(), (int)generic.size()}};
    for (int i = 1; i < argc; i++) {
        const Plan p = plan(parse(argv[i]), tabs, 4);
        char name[160] = "";
        if (p.row) format_name(*p.row, name, sizeof name);
        printf("{\"name\": \"%s\", \"threads\": %d, \"lds\": %d, \"ws_valid_after\": %s, \"pair_swap_bit\": %d, \"err\": \"%s\"}\n", name, p.threads, p.lds,
               p.ws_valid_after ? "true" : "false", p.pair_swap_bit, p.err ? p.err : "");
    }
    return 0;
}
