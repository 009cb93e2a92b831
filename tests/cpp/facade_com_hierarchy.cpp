// The whole-body hierarchy of reference tests/sp_test/regulation_test.cpp:81-129 as the harness writes it, against the drop-in facade
// include/dwbc_amd.hpp: rot_z = 0, the synthetic "COM" link 6D on level 0, pelvis and upper-body rotation, both hands on level 3
// (two AddTaskSpace(3, ...) calls, a 12-vector f*), four registered contacts with the feet raised, no torque limit.
// Prints the three torque vectors and getContactForce as JSON for tests/test_facade_com_hierarchy.py.
#include <cstdio>
#include <cmath>
#include <string>

#include "dwbc_amd.hpp"

using namespace DWBC;

static void print_vec(const char *name, const Vec &v, bool last = false) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%.17g", i ? ", " : "", v[i]);
    printf("]%s\n", last ? "" : ",");
}

// rd2_.link_[0].rotm * v
static void rotate(const Mat &R, double *v) {
    const double a[3] = {v[0], v[1], v[2]};
    for (int i = 0; i < 3; i++) v[i] = R(i, 0) * a[0] + R(i, 1) * a[1] + R(i, 2) * a[2];
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: facade_com_hierarchy <urdf>\n"); return 2; }
    bool contact1 = true, contact2 = true, contact3 = false;
    const double rot_z = 0;
    bool use_hqp = true;
    std::string desired_control_target = "COM";
    std::string desired_control_target2 = "pelvis_link";
    std::string desired_control_target3 = "upperbody_link";
    std::string desired_control_target4 = "L_Wrist2_Link";
    std::string desired_control_target5 = "R_Wrist2_Link";
    Vec fstar_1{0.5, 0.3, 0.2, 0.12, -0.11, 0.05};

    RobotData rd2_;
    rd2_.LoadModelData(argv[1], true, false);
    if (rd2_.system_dof_ != 39) { fprintf(stderr, "model load failed\n"); return 3; }
    // AngleAxis(0, X) * AngleAxis(0, Y) * AngleAxis(rot_z, Z)
    const double qx = 0, qy = 0, qz = std::sin(rot_z / 2), qw = std::cos(rot_z / 2);
    Vec q2{0, 0, 0, qx, qy, qz,
           0.0, 0.0, -0.24, 0.6, -0.36, 0.0,
           0.0, 0.0, -0.24, 0.6, -0.36, 0.0,
           0, 0, 0,
           0.3, 0.3, 1.5, -1.27, -1, 0, -1, 0,
           0, 0,
           -0.3, -0.3, -1.5, 1.27, 1, 0, 1, 0, qw};
    Vec q2dot(39, 0.0), q2ddot(39, 0.0);

    bool verbose = false;
    rd2_.UpdateKinematics(q2, q2dot, q2ddot);
    rd2_.AddContactConstraint("l_ankleroll_link", CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.13, 0.06, verbose);
    rd2_.AddContactConstraint("r_ankleroll_link", CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.13, 0.06, verbose);
    rd2_.AddContactConstraint(23, CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.04, 0.04);
    rd2_.AddContactConstraint(31, CONTACT_6D, Vec3(0.03, 0, -0.1585), Vec3(0, 0, 1), 0.04, 0.04);

    rd2_.AddTaskSpace(0, TASK_LINK_6D, desired_control_target.c_str(), Vec3(), verbose);
    rd2_.AddTaskSpace(1, TASK_LINK_ROTATION, desired_control_target2.c_str(), Vec3(), verbose);
    rd2_.AddTaskSpace(2, TASK_LINK_ROTATION, desired_control_target3.c_str(), Vec3(), verbose);
    rd2_.AddTaskSpace(3, TASK_LINK_6D, desired_control_target4.c_str(), Vec3(), verbose);
    rd2_.AddTaskSpace(3, TASK_LINK_6D, desired_control_target5.c_str(), Vec3(), verbose);

    rd2_.SetContact(contact1, contact2, contact3, false);
    int ok_c = rd2_.CalcContactConstraint();

    rotate(rd2_.link_[0].rotm, &fstar_1[0]);
    rotate(rd2_.link_[0].rotm, &fstar_1[3]);

    Vec f_star3(12, 0.0);
    for (int i = 0; i < 6; i++) { f_star3[i] = 0.5 * fstar_1[i]; f_star3[6 + i] = 0.2 * fstar_1[i]; }
    Vec f_star0{-2, -2.2, 0.2, 0.5, 0.4, -0.6};

    rd2_.SetTaskSpace(0, f_star0);
    rd2_.SetTaskSpace(1, Vec{fstar_1[3], fstar_1[4], fstar_1[5]});
    rd2_.SetTaskSpace(2, Vec{-fstar_1[3], -fstar_1[4], -fstar_1[5]});
    rd2_.SetTaskSpace(3, f_star3);

    rd2_.CalcGravCompensation();
    int ok_t = rd2_.CalcTaskControlTorque(use_hqp, true);
    int ok_r = rd2_.CalcContactRedistribute(use_hqp, true);

    printf("{\n");
    printf("\"com_id\": %d,\n", rd2_.getLinkID("COM"));
    printf("\"dims\": [%d, %d, %d, %d],\n", (int)rd2_.ts_.size(), rd2_.ts_[0].task_dof_, rd2_.ts_[3].task_dof_, (int)rd2_.contact_dof_);
    printf("\"ok\": [%d, %d, %d],\n", ok_c, ok_t, ok_r);
    print_vec("pelvis_rotm", rd2_.link_[0].rotm.d);
    print_vec("torque_grav_", rd2_.torque_grav_);
    print_vec("torque_task_", rd2_.torque_task_);
    print_vec("torque_contact_", rd2_.torque_contact_);
    Vec total(rd2_.model_dof_);
    for (unsigned i = 0; i < rd2_.model_dof_; i++) total[i] = rd2_.torque_grav_[i] + rd2_.torque_task_[i] + rd2_.torque_contact_[i];
    print_vec("contact_force", rd2_.getContactForce(total), true);
    printf("}\n");
    return 0;
}
