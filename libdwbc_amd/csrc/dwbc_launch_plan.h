// dwbc_launch_plan.h -- which build of the cycle kernel serves a solve (and which kernel a redistribution of a caller-supplied torque, a link query, a gravity compensation, the dynamics of UpdateKinematics, the contact space of CalcContactConstraint, the task space of CalcTaskSpace or one level's task QP of CalcSingleTaskTorqueWithQP):
// the table row of every launchable kernel and the one function that picks among them.  Host only, no HIP header: dwbc_kernels.h emits the rows (fp64, fp32 and pack builds alike),
// dwbc_capi.hip launches what plan() returns and reports it, tests/cpp/launch_plan.cpp runs plan() over a hand-written table.
// The namespace is not `dwbc`: the fp32 build renames that one.
#pragma once
#include <cstdio>

namespace dwbc_plan {

enum Arith { kDouble = 0, kFloat = 1 };
// full-model cycle, reduced (centroidal) dynamics, general-contact cycle, redistribution of a caller-supplied torque (dwbc_redistribute.h),
// link poses / velocities / Jacobians on their own (dwbc_link_query.h), gravity compensation alone or before such a redistribution
// (dwbc_redistribute.h, GRAV = true)
// the dynamics half of UpdateKinematics on its own (dwbc_dynamics.h)
// SetContact + CalcContactConstraint on their own (dwbc_contact_space.h)
// SetTaskSpace + CalcTaskSpace on their own (dwbc_task_space.h)
// CalcSingleTaskTorqueWithQP for one task level on its own (dwbc_task_qp.h)
enum Kind { kCycle = 0, kReduced = 1, kGc = 2, kRedist = 3, kLinkQuery = 4, kGravComp = 5, kDynamics = 6, kContactSpace = 7, kTaskSpace = 8, kTaskQp = 9 };
enum : unsigned {
    kWide = 1,       // no register cap (one wave per SIMD): batches of at most 4 instances per CU
    kLean = 2,       // EXTRAS = false: none of the optional paths
    kCompact = 4,    // the 20 KB LDS map (Lds3)
    kTwoWave = 8,    // two wavefronts per instance (dwbc_cycle2p.h)
    kWideTasks = 16, // general-contact cycle sized for task levels of up to 12 dof (TG = 12)
    kInstModel = 32  // built with DWBC_INST_MODEL (namespace dwbc_im): BatchIO::body holds one body table per instance
};

struct Row {  // one launchable kernel
    int n, nb;  // model size (system dof, bodies)
    int nlv;    // task levels its LDS map is sized for (0: any)
    int topo;   // 0: any tree, 1: TopoTocabi's constant tree, 2: the one tree a pack was compiled for (TopoPack)
    int arith, kind;
    unsigned flavour;
    const void *fn;
    int lds;      // dynamic LDS bytes of fn
    int threads;  // per instance (= per workgroup)
    const char *base, *tail;  // base<tail> is the name a profiler prints for fn
};
struct Table {
    const Row *rows;
    int count;
};

struct Request {
    int n, nb, levels;
    int topo;         // Setup::topo_kind of the model
    bool tree_match;  // the model's parent table is the one the offered TopoPack rows were compiled for
    int arith, B, n_cu;
    bool reduced;
    int max_active;   // simultaneously active contacts the batch is set up for
    bool wide_tasks;  // a task level of more than six dof
    // what the lean build cannot serve
    bool hqp, warm;
    int n_traj;
    bool has_com_task;
    int n_custom;
    bool dump_on;
    // environment: DWBC_NO_WIDE, DWBC_NO_PAIR, DWBC_NO_LEAN, DWBC_PAIR_ALWAYS (development: the two-wave kernel at any batch size),
    // DWBC_PAIR_SWAP_BIT (-1: unset)
    bool no_wide, no_pair, no_lean, pair_always;
    int pair_swap_bit;
    // not a cycle: CalcContactRedistribute(torque_input, hqp, init) on a caller-supplied torque (dwbc_batch_redistribute); of the members
    // above it reads the model, arith, max_active and hqp
    bool redistribute = false;
    // the batch carries per-instance torque limits and contact cone constants (BatchIO::inst_par): every kernel of the table reads them where
    // it fills a QP row, so no route changes; what has no QP rows to put them in is refused
    bool inst_par = false;
    // not a cycle either: UpdateKinematics on its own for a set of queried links (dwbc_batch_update_kinematics); of the members above it reads
    // the model and arith
    bool link_query = false;
    // not a cycle either: CalcGravCompensation on its own, or ahead of the redistribution of a command on top of it
    // (dwbc_batch_grav_compensation, dwbc_batch_redistribute with DWBC_REDIST_ADD_GRAVITY); of the members above it reads the model, arith
    // and max_active (the caller plans the redistribution request as well where there is one: its refusals come first)
    bool grav_comp = false;
    // not a cycle either: the dynamics half of UpdateKinematics on its own (dwbc_batch_update_dynamics); of the members above it reads the
    // model and arith
    bool dynamics = false;
    // not a cycle either: SetContact + CalcContactConstraint on their own (dwbc_batch_calc_contact_constraint); of the members above it reads
    // the model, arith, max_active and n_contacts
    bool contact_space = false;
    int n_contacts = 0;  // registered contacts of the batch (read by the contact-space request alone)
    // not a cycle either: SetTaskSpace + CalcTaskSpace on their own (dwbc_batch_calc_task_space); of the members above it reads the model,
    // arith, max_active, levels, wide_tasks and n_custom
    bool task_space = false;
    // the batch carries one body table per instance (dwbc_batch_set_instance_model / dwbc_batch_bind_instance_model): a request is served by
    // rows with kInstModel and by no others, so every route below picks the dwbc_im:: twin of the kernel it would pick without the record
    bool inst_model = false;
    // not a cycle either: CalcSingleTaskTorqueWithQP for one task level on its own (dwbc_batch_calc_single_task_torque_qp); of the members
    // above it reads the model, arith, max_active, levels, wide_tasks and n_custom (per-instance parameters shape its QP rows as they do the
    // cycle's: no route changes)
    bool task_qp = false;
};

struct Plan {
    const Row *row;  // nullptr: refused, err says why
    int threads, lds;
    bool ws_valid_after;  // the launch leaves every QP's working set in the diagnostics record (DG_QP_ACT): the next solve may start warm
    int pair_swap_bit;    // BatchIO::pair_swap_bit of the launch (-1 unless the two-wave kernel runs)
    const char *err;
};

inline int format_name(const Row &r, char *buf, size_t len) { return snprintf(buf, len, "%s<%s>", r.base, r.tail); }

// the rows of one kind a request may use: those of the first table that holds any (built in before a pack of the model's own tree
// before a generic pack: the caller lists the tables in that order), and of these the ones built for the model's tree if there are such
struct Candidates {
    const Request &q;
    int kind;
    const Table *tab = nullptr;
    bool specific = false;
    bool usable(const Row &r) const {
        return r.n == q.n && r.nb == q.nb && r.arith == q.arith && r.kind == kind && (r.nlv == 0 || r.nlv == q.levels) &&
               ((r.flavour & kInstModel) != 0) == q.inst_model && (r.topo == 0 || (r.topo == 2 ? q.tree_match : r.topo == q.topo));
    }
    Candidates(const Request &q_, int kind_, const Table *tabs, int n_tabs) : q(q_), kind(kind_) {
        for (int t = 0; t < n_tabs && !tab; t++)
            for (int i = 0; i < tabs[t].count; i++)
                if (usable(tabs[t].rows[i])) {
                    tab = &tabs[t];
                    specific = specific || tabs[t].rows[i].topo != 0;
                }
    }
    const Row *pick(unsigned mask, unsigned want) const {  // the row whose flavour bits under `mask` are `want`
        for (int i = 0; tab && i < tab->count; i++) {
            const Row &r = tab->rows[i];
            if (usable(r) && (r.topo != 0) == specific && (r.flavour & mask) == want) return &r;
        }
        return nullptr;
    }
};

// what a request with a per-instance body table is refused with (after every refusal the same request meets without the record)
constexpr const char *kInstModelReduced = "per-instance model: not built on the reduced dynamics path (drop the record with dwbc_batch_set_instance_model(b, NULL))";
constexpr const char *kInstModelGc = "per-instance model: not built for three active contacts or task levels of more than 6 dof (the general-contact kernel has no such build)";
constexpr const char *kInstModelNone =
    "per-instance model: no kernel for this request (built for fp64 batches on TOCABI's constant tree: the full-model cycle of 1 to 4 task levels on every "
    "launch route, and the redistribution, gravity-compensation, link-query, dynamics, contact-space and task-space launches)";

inline Plan plan(const Request &q, const Table *tabs, int n_tabs) {
    Plan p{nullptr, 0, 0, false, -1, nullptr};
    auto refuse = [&](const char *why) {
        p.err = why;
        return p;
    };
    // with a record: whatever refuses the request without it refuses it first, in the same words
    if (q.inst_model) {
        Request base = q;
        base.inst_model = false;
        const Plan pb = plan(base, tabs, n_tabs);
        if (!pb.row) return pb;
    }
    auto none = [&](const char *why) { return refuse(q.inst_model ? kInstModelNone : why); };
    auto run = [&](const Row *r, bool ws_valid_after) {
        p.row = r;
        p.threads = r->threads;
        p.lds = r->lds;
        p.ws_valid_after = ws_valid_after;
        return p;
    };
    // link query: one kernel for any tree of its size, whatever the batch size, the task set-up or the cycle's options are (it reads the state alone)
    if (q.link_query) {
        if (q.arith == kFloat) return refuse("link query: fp64 batches only");
        const Row *r = Candidates(q, kLinkQuery, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no link-query kernel for this model (built in for TOCABI's size, any tree; kernel packs do not carry one)");
        return run(r, false);
    }
    // dynamics of UpdateKinematics: one kernel per model size and tree, whatever the batch size, the contact and task set-up or the cycle's
    // options are (it reads the state alone)
    if (q.dynamics) {
        if (q.arith == kFloat) return refuse("dynamics: fp64 batches only");
        const Row *r = Candidates(q, kDynamics, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no dynamics kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)");
        return run(r, false);
    }
    // gravity compensation: planned like the redistribution below, whatever the batch size, the levels or the cycle's options are
    if (q.grav_comp) {
        if (q.arith == kFloat) return refuse("gravity compensation: fp64 batches only");
        if (q.max_active > 2) return refuse("gravity compensation: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))");
        const Row *r = Candidates(q, kGravComp, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no gravity-compensation kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)");
        return run(r, false);
    }
    // redistribution of a caller-supplied torque: one lean kernel, whatever the batch size or the task set-up (it runs no task level and
    // starts its one QP cold)
    if (q.redistribute) {
        if (q.arith == kFloat) return refuse("redistribution of a supplied torque: fp64 batches only");
        if (q.max_active > 2) return refuse("redistribution of a supplied torque: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))");
        const Row *r = Candidates(q, kRedist, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no redistribution kernel for this model (built in for TOCABI's size and tree; kernel packs do not carry one)");
        if (!q.hqp) return refuse("redistribution of a supplied torque: hqp = true only (the closed form of src/dwbc.cpp:1570-1619 is not built for a supplied torque)");
        return run(r, false);
    }
    // contact space of CalcContactConstraint: one kernel per model size and tree, whatever the batch size, the levels or the cycle's options are
    if (q.contact_space) {
        if (q.arith == kFloat) return refuse("contact space: fp64 batches only");
        if (q.max_active > 2) return refuse("contact space: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))");
        const Row *r = Candidates(q, kContactSpace, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no contact-space kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)");
        if (q.n_contacts < 1) return refuse("contact space: no contact constraint (call dwbc_batch_add_contact first)");
        return run(r, false);
    }
    // task space of CalcTaskSpace: one kernel per model size and tree, whatever the batch size, hqp, warm or the dump record are
    if (q.task_space) {
        if (q.arith == kFloat) return refuse("task space: fp64 batches only");
        if (q.max_active > 2) return refuse("task space: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))");
        if (q.wide_tasks) return refuse("task space: task levels of at most 6 dof");
        if (q.n_custom > 0) return refuse("task space: TASK_CUSTOM levels are not built (their J_task is the caller's own)");
        const Row *r = Candidates(q, kTaskSpace, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no task-space kernel for this model (built in for TOCABI's size, any tree; a kernel pack carries one for its size)");
        if (q.levels < 1) return refuse("task space: no task level (call dwbc_batch_add_task first)");
        return run(r, false);
    }
    // one level's task QP of CalcSingleTaskTorqueWithQP: one kernel per model size and tree, whatever the batch size, hqp, warm or the dump record are
    if (q.task_qp) {
        if (q.arith == kFloat) return refuse("single-level task QP: fp64 batches only");
        if (q.max_active > 2) return refuse("single-level task QP: two simultaneously active contacts at most (call dwbc_batch_set_max_active_contacts(b, 2))");
        if (q.wide_tasks) return refuse("single-level task QP: task levels of at most 6 dof");
        if (q.n_custom > 0) return refuse("single-level task QP: TASK_CUSTOM levels are not built (their J_task is the caller's own)");
        const Row *r = Candidates(q, kTaskQp, tabs, n_tabs).pick(0u, 0u);
        if (!r) return none("no single-level task-QP kernel for this model (built in for TOCABI's size, any tree; kernel packs do not carry one)");
        if (q.levels < 1) return refuse("single-level task QP: no task level (call dwbc_batch_add_task first)");
        return run(r, false);
    }
    // three active contacts, or a task level of more than six dof: the general-contact kernel (lean scope: link tasks and the
    // synthetic COM link; QPs start cold and keep no working sets)
    if (q.max_active > 2 || q.wide_tasks) {
        if (q.inst_model) return refuse(kInstModelGc);
        if (q.reduced) return refuse("three active contacts / task levels of more than 6 dof: not built on the reduced dynamics path");
        if (q.arith == kFloat) return refuse("three active contacts / task levels of more than 6 dof: fp64 batches only");
        const Candidates gc(q, kGc, tabs, n_tabs);
        const Row *r = gc.pick(kWideTasks, 0);
        if (!r) return none("no general-contact kernel for this model size (built in for TOCABI; kernel packs carry one for models of at most 40 dof)");
        if (q.wide_tasks && !(r = gc.pick(kWideTasks, kWideTasks))) return refuse("task levels of more than 6 dof: built in for TOCABI's size only");
        if (!q.hqp) return refuse("three active contacts / task levels of more than 6 dof: hqp = true only (the reference's closed-form redistribution is written for two contacts, src/dwbc.cpp:1570-1619)");
        if (q.n_traj > 0 || q.n_custom > 0 || q.dump_on)
            return refuse("three active contacts / task levels of more than 6 dof: link and COM tasks with f* from SetTaskSpace only (no trajectories, no TASK_CUSTOM levels, no dump record)");
        return run(r, false);
    }
    if (q.inst_model && q.reduced) return refuse(kInstModelReduced);
    const Candidates c(q, q.reduced ? kReduced : kCycle, tabs, n_tabs);
    if (!c.tab) return none(q.arith == kFloat ? "no fp32 kernel for this model / number of task levels" : "no kernel for this model / number of task levels");
    if (q.arith == kFloat && q.dump_on) return refuse("the dump record is not available on DWBC_F32 batches");
    // the lean build (EXTRAS = false) serves every launch that uses none of the optional paths
    const bool lean_asked = q.hqp && !q.warm && q.n_traj == 0 && !q.has_com_task && q.n_custom == 0 && !q.dump_on && !q.no_lean;
    const bool lean = lean_asked && c.pick(kLean, kLean);
    const bool wide = q.B <= 4 * q.n_cu && !q.no_wide && c.pick(kWide, kWide);
    // the extras build of the full cycle leaves the working sets behind.  (fp32 batches go by the request alone, as they always have:
    // a tree without a lean build starts warm one solve later.)
    const bool ws_valid_after = q.arith == kFloat ? !lean_asked : (!lean && !q.reduced);
    // two waves per instance, side chains on the helper wave: the lean fp64 cycle of small batches (one instance per SIMD)
    const Row *r = nullptr;
    if ((wide || q.pair_always) && lean && !q.reduced && q.arith == kDouble && !q.no_pair) r = c.pick(kTwoWave, kTwoWave);
    const bool two_wave = r != nullptr;
    if (!r) r = c.pick(kWide | kLean | kTwoWave, (wide ? kWide : 0u) | (lean ? kLean : 0u));
    if (!r) return none("no kernel for this model / number of task levels");
    // per-instance parameters shape QP rows: the reduced path refuses a torque limit already, and the closed form of hqp = false knows neither
    // limits nor cones (a randomisation that is silently ignored is worse than a refusal)
    if (q.inst_par && q.reduced) return refuse("per-instance parameters: not built on the reduced dynamics path (drop them with dwbc_batch_set_instance_params(b, NULL))");
    if (q.inst_par && !q.hqp) return refuse("per-instance parameters: hqp = true only (the closed form of hqp = false reads neither torque limits nor contact cones)");
    if (two_wave) p.pair_swap_bit = q.pair_swap_bit;
    return run(r, ws_valid_after);
}

}  // namespace dwbc_plan
