// RobotData::CalcContactRedistribute(torque_input, hqp, init) through the drop-in facade include/dwbc_amd.hpp on a model that runs through a
// kernel pack (the TOCABI fixture with the head joints fixed: 37 dof / 32 bodies), as tests/cpp/facade_redistribute.cpp does on TOCABI.
//   facade_redistribute_pack <urdf> <system dof> <q: system dof + 1 values> <torque_input: system dof - 6 values>
// The driver (tests/test_redistribute_packs_gpu.py) computes the state, the torque and the expected answers.  Prints JSON.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "dwbc_amd.hpp"

using namespace DWBC;

static void print_vec(const char *name, const Vec &v, bool last = false) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%.17g", i ? ", " : "", v[i]);
    printf("]%s\n", last ? "" : ",");
}

int main(int argc, char **argv) {
    if (argc < 3) { fprintf(stderr, "usage: facade_redistribute_pack <urdf> <system dof> <q> <torque_input>\n"); return 2; }
    const int n = atoi(argv[2]), m = n - 6;
    if (n < 7 || argc != 3 + (n + 1) + m) { fprintf(stderr, "expected %d values behind the system dof\n", n + 1 + m); return 2; }
    RobotData rd_;
    rd_.LoadModelData(argv[1], true, false);
    if ((int)rd_.system_dof_ != n) { fprintf(stderr, "model load failed (system dof %d)\n", (int)rd_.system_dof_); return 3; }
    Vec q(n + 1), qdot(n, 0.0), qddot(n, 0.0), tin(m);
    for (int i = 0; i < n + 1; i++) q[i] = atof(argv[3 + i]);
    for (int i = 0; i < m; i++) tin[i] = atof(argv[3 + n + 1 + i]);
    rd_.UpdateKinematics(q, qdot, qddot);
    rd_.AddContactConstraint("L_AnkleRoll_Link", CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.15, 0.075);
    rd_.AddContactConstraint("R_AnkleRoll_Link", CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.15, 0.075);
    rd_.AddTaskSpace(0, TASK_LINK_6D, 0, Vec3());
    rd_.AddTaskSpace(1, TASK_LINK_ROTATION, "upperbody_link", Vec3());
    rd_.SetTorqueLimit(Vec(rd_.model_dof_, 300.0));
    rd_.UpdateKinematics(q, qdot, qddot);
    rd_.SetContact(true, true);
    const int ok_c = rd_.CalcContactConstraint();
    rd_.SetTaskSpace(0, Vec{0.1, 4.0, 0.1, 0.1, -0.1, 0.1});
    rd_.SetTaskSpace(1, Vec{0.1, -0.1, 0.1});
    rd_.CalcGravCompensation();
    const int ok_t = rd_.CalcTaskControlTorque(true);  // torque_contact_ = NwJw contact_qp_ of the last level: the overload adds to it
    const Vec tc_before = rd_.torque_contact_;
    const int ok_p = rd_.CalcContactRedistribute(tin, true, true);
    Vec tc(m);
    for (int i = 0; i < m; i++) tc[i] = rd_.torque_contact_[i] - tc_before[i];
    const Vec cf = rd_.cf_redis_qp_;
    printf("{\n\"ok\": [%d, %d, %d],\n\"model_dof\": %d,\n", ok_c, ok_t, ok_p, (int)rd_.model_dof_);
    print_vec("torque_contact_increment", tc);
    print_vec("cf_redis_qp_", cf, true);
    printf("}\n");
    return 0;
}
