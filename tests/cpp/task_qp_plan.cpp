// task_qp_plan.cpp -- dwbc_plan::plan() (libdwbc_amd/csrc/dwbc_launch_plan.h) for CalcSingleTaskTorqueWithQP of one task level on its own
// (Request::task_qp), over a hand-written table: TOCABI's compact lean cycle row, its extras row, its redistribution, gravity-compensation,
// link-query, dynamics, contact-space, task-space and task-QP rows in fp64 (the last two on its own tree and on any), the general-contact
// row, the cycle row alone in fp32, a per-instance-model cycle row, and a 37-dof / 32-body pack that carries every lean row but the
// task-QP one (no pack does).
// No GPU, no HIP.  Every argument is one request, `key=value,key=value` over the defaults below; the answer to each is one JSON line.
// Driven by tests/test_task_qp_plan.py.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../libdwbc_amd/csrc/dwbc_launch_plan.h"

using namespace dwbc_plan;

static char g_kernels[32];

int main(int argc, char **argv) {
    static_assert(kContactSpace == 7 && kTaskSpace == 8 && kTaskQp == 9, "appended to Kind");
    const std::vector<Row> f64 = {
        Row{39, 34, 2, 1, kDouble, kCycle, kLean | kCompact, &g_kernels[0], 20432, 64, "dwbc::dwbc_cycle_kernel_v2", "39, 34, 2, 64, false, dwbc::TopoTocabi, true"},
        Row{39, 34, 2, 1, kDouble, kCycle, 0u, &g_kernels[1], 31000, 64, "dwbc::dwbc_cycle_kernel_v2", "39, 34, 2, 64, true, dwbc::TopoTocabi"},
        Row{39, 34, 0, 1, kDouble, kRedist, 0u, &g_kernels[2], 20432, 64, "dwbc::dwbc_redistribute_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 1, kDouble, kGravComp, 0u, &g_kernels[3], 20432, 64, "dwbc::dwbc_gravcomp_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 0, kDouble, kLinkQuery, 0u, &g_kernels[4], 13000, 64, "dwbc::dwbc_link_query_kernel", "39, 34"},
        Row{39, 34, 0, 1, kDouble, kDynamics, 0u, &g_kernels[5], 15536, 64, "dwbc::dwbc_dynamics_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 1, kDouble, kContactSpace, 0u, &g_kernels[6], 20432, 64, "dwbc::dwbc_contact_space_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 0, kDouble, kGc, 0u, &g_kernels[7], 80000, 64, "dwbc::dwbc_cycle_kernel_gc", "39, 34, 64, 6"},
        Row{39, 34, 0, 1, kDouble, kTaskSpace, 0u, &g_kernels[8], 38656, 64, "dwbc::dwbc_task_space_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 0, kDouble, kTaskSpace, 0u, &g_kernels[9], 38656, 64, "dwbc::dwbc_task_space_kernel", "39, 34, dwbc::TopoGeneric"},
        Row{39, 34, 0, 1, kDouble, kTaskQp, 0u, &g_kernels[16], 37872, 64, "dwbc::dwbc_task_qp_kernel", "39, 34, dwbc::TopoTocabi"},
        Row{39, 34, 0, 0, kDouble, kTaskQp, 0u, &g_kernels[17], 37872, 64, "dwbc::dwbc_task_qp_kernel", "39, 34, dwbc::TopoGeneric"},
        Row{39, 34, 2, 1, kDouble, kCycle, kInstModel, &g_kernels[18], 31000, 64, "dwbc_im::dwbc_cycle_kernel_v2", "39, 34, 2, 64, true, dwbc_im::TopoTocabi"},
        Row{39, 34, 0, 1, kDouble, kTaskSpace, kInstModel, &g_kernels[19], 38656, 64, "dwbc_im::dwbc_task_space_kernel", "39, 34, dwbc_im::TopoTocabi"},
    };
    const std::vector<Row> f32 = {
        Row{39, 34, 2, 1, kFloat, kCycle, 0u, &g_kernels[10], 31000, 64, "dwbc_f32::dwbc_cycle_kernel_v2", "39, 34, 2, 64, true, dwbc_f32::TopoTocabi"},
    };
    const std::vector<Row> pack = {
        Row{37, 32, 2, 0, kDouble, kCycle, 0u, &g_kernels[11], 29000, 64, "dwbc::dwbc_cycle_kernel_v2", "37, 32, 2, 64, true, dwbc::TopoGeneric"},
        Row{37, 32, 0, 0, kDouble, kContactSpace, 0u, &g_kernels[12], 19488, 64, "dwbc::dwbc_contact_space_kernel", "37, 32, dwbc::TopoGeneric"},
        Row{37, 32, 0, 0, kDouble, kTaskSpace, 0u, &g_kernels[13], 36944, 64, "dwbc::dwbc_task_space_kernel", "37, 32, dwbc::TopoGeneric"},
    };
    const Table tabs[3] = {{f64.data(), (int)f64.size()}, {f32.data(), (int)f32.size()}, {pack.data(), (int)pack.size()}};
    for (int i = 1; i < argc; i++) {
        Request q{};
        q.n = 39, q.nb = 34, q.levels = 2, q.topo = 1, q.arith = kDouble, q.B = 250, q.n_cu = 256, q.max_active = 2, q.hqp = true, q.pair_swap_bit = -1, q.n_contacts = 2;
        std::string s(argv[i]);
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
            else if (k == "max_active") q.max_active = v;
            else if (k == "wide_tasks") q.wide_tasks = v;
            else if (k == "n_custom") q.n_custom = v;
            else if (k == "hqp") q.hqp = v;
            else if (k == "warm") q.warm = v;
            else if (k == "dump_on") q.dump_on = v;
            else if (k == "inst_par") q.inst_par = v;
            else if (k == "redistribute") q.redistribute = v;
            else if (k == "grav_comp") q.grav_comp = v;
            else if (k == "link_query") q.link_query = v;
            else if (k == "dynamics") q.dynamics = v;
            else if (k == "contact_space") q.contact_space = v;
            else if (k == "task_space") q.task_space = v;
            else if (k == "task_qp") q.task_qp = v;
            else if (k == "inst_model") q.inst_model = v;
            else if (k == "n_contacts") q.n_contacts = v;
            else if (!kv.empty()) {
                fprintf(stderr, "unknown key '%s'\n", k.c_str());
                return 2;
            }
        }
        const Plan p = plan(q, tabs, 3);
        char name[160] = "";
        if (p.row) format_name(*p.row, name, sizeof name);
        printf("{\"name\": \"%s\", \"threads\": %d, \"lds\": %d, \"ws_valid_after\": %s, \"err\": \"%s\"}\n", name, p.threads, p.lds, p.ws_valid_after ? "true" : "false",
               p.err ? p.err : "");
    }
    return 0;
}
