// RobotData::CalcContactRedistribute(torque_input, hqp, init) (reference include/dwbc.h:297, src/dwbc.cpp:1377-1568) through the drop-in
// facade include/dwbc_amd.hpp, on the CASE 1 state of reference tests/dwbc_test.cpp:29-131.
//   facade_redistribute <urdf> <33 torques>
// (a) the cycle's own torque handed back in: the same torque_contact_ as the no-argument overload leaves;
// (b) the 33 torques of the command line (the driver perturbs the cycle's torque along the contact null space): torque_contact_ increment,
//     cf_redis_qp_ and getContactForce before / after, for tests/test_facade_redistribute.py to compare with the restatement;
// (c) an Eigen-like vector type, hqp = false and a vector of the wrong size.  Prints JSON.
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

// what the facade needs of an Eigen vector
struct EigenLike {
    std::vector<double> s;
    const double *data() const { return s.data(); }
    long size() const { return (long)s.size(); }
    long rows() const { return (long)s.size(); }
};

int main(int argc, char **argv) {
    if (argc != 2 + 33) { fprintf(stderr, "usage: facade_redistribute <urdf> <33 torques>\n"); return 2; }
    RobotData rd_;
    rd_.LoadModelData(argv[1], true, false);
    if (rd_.system_dof_ != 39) { fprintf(stderr, "model load failed\n"); return 3; }
    Vec q(rd_.system_dof_ + 1, 0.0), qdot(rd_.system_dof_, 0.0), qddot(rd_.system_dof_, 0.0);
    const double q1[40] = {0, 0, 0.92983, 0, 0, 0, 0.0, 0.0, -0.24, 0.6, -0.36, 0.0, 0.0, 0.0, -0.24, 0.6, -0.36, 0.0, 0, 0, 0,
                           0.3, 0.3, 1.5, -1.27, -1, 0, -1, 0, 0, 0, -0.3, -0.3, -1.5, 1.27, 1, 0, 1, 0, 1};
    for (int i = 0; i < 40; i++) q[i] = q1[i];
    rd_.UpdateKinematics(q, qdot, qddot);
    rd_.AddContactConstraint(6, CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.15, 0.075);
    rd_.AddContactConstraint(12, CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.15, 0.075);
    rd_.AddTaskSpace(0, TASK_LINK_6D, 0, Vec3());
    rd_.AddTaskSpace(1, TASK_LINK_ROTATION, "upperbody_link", Vec3());
    rd_.SetTorqueLimit(Vec(rd_.model_dof_, 300.0));
    rd_.UpdateKinematics(q, qdot, qddot);
    rd_.SetContact(true, true);
    const int ok_c = rd_.CalcContactConstraint();
    rd_.SetTaskSpace(0, Vec{0.1, 4.0, 0.1, 0.1, -0.1, 0.1});
    rd_.SetTaskSpace(1, Vec{0.1, -0.1, 0.1});
    rd_.CalcGravCompensation();
    const unsigned m = rd_.model_dof_;
    auto total = [&]() {
        Vec t(m);
        for (unsigned i = 0; i < m; i++) t[i] = rd_.torque_grav_[i] + rd_.torque_task_[i] + rd_.torque_contact_[i];
        return t;
    };

    // (a) the two overloads on the cycle's own torque
    const int ok_t = rd_.CalcTaskControlTorque(true);
    const int ok_r0 = rd_.CalcContactRedistribute(true);
    const Vec tc_noarg = rd_.torque_contact_;
    rd_.CalcTaskControlTorque(true);  // torque_contact_ back to NwJw contact_qp_ of the last level
    const Vec tc_before = rd_.torque_contact_;
    const int ok_r1 = rd_.CalcContactRedistribute(total());
    const Vec tc_arg = rd_.torque_contact_;

    // (b) the driver's torque
    Vec tin(m);
    for (unsigned i = 0; i < m; i++) tin[i] = atof(argv[2 + i]);
    rd_.CalcTaskControlTorque(true);
    const int ok_p = rd_.CalcContactRedistribute(tin, true, true);
    Vec dt(m), tout(m);
    for (unsigned i = 0; i < m; i++) { dt[i] = rd_.torque_contact_[i] - tc_before[i]; tout[i] = tin[i] + dt[i]; }
    const Vec cf = rd_.cf_redis_qp_;
    const Vec w0 = rd_.getContactForce(tin), w1 = rd_.getContactForce(tout);

    // (c) an Eigen-like vector, then the refusals
    rd_.CalcTaskControlTorque(true);
    EigenLike ev{tin};
    const int ok_e = rd_.CalcContactRedistribute(ev);
    Vec dte(m);
    for (unsigned i = 0; i < m; i++) dte[i] = rd_.torque_contact_[i] - tc_before[i];
    const int ok_nohqp = rd_.CalcContactRedistribute(tin, false);
    const int ok_size = rd_.CalcContactRedistribute(Vec(m - 1, 0.0));

    printf("{\n\"ok\": [%d, %d, %d, %d, %d, %d, %d, %d],\n", ok_c, ok_t, ok_r0, ok_r1, ok_p, ok_e, ok_nohqp, ok_size);
    print_vec("torque_contact_noarg", tc_noarg);
    print_vec("torque_contact_arg", tc_arg);
    print_vec("delta", dt);
    print_vec("delta_eigen_like", dte);
    print_vec("cf_redis_qp_", cf);
    print_vec("wrench_in", w0);
    print_vec("wrench_out", w1, true);
    printf("}\n");
    return 0;
}
