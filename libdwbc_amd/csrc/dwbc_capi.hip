// dwbc_capi.hip -- C-ABI (include/dwbc_batch.h) + kernel launch for the MI355X-native batched libdwbc hot path.
// gfx950 only.  No CPU fallback: every compute entry point needs a HIP device and fails loudly without one.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <vector>

#include "dwbc_kernels.h"
#include "dwbc_capi_internal.h"
#include "dwbc_setup.h"

using namespace dwbc;

extern "C" const dwbc_plan::Row *dwbc_f32_rows(int *count);  // launch table of the fp32 build (dwbc_kernels_f32.hip)
extern "C" const dwbc_plan::Row *dwbc_task_space_rows(int *count);  // the built-in task-space kernels (dwbc_kernels_task_space.hip)
extern "C" const dwbc_plan::Row *dwbc_task_qp_rows(int *count);  // the built-in single-level task-QP kernels (dwbc_kernels_task_qp.hip)
// the kernels that read one body table per instance (dwbc_kernels_im.h), split over translation units of their own
extern "C" const dwbc_plan::Row *dwbc_im_rows_l1(int *count);
extern "C" const dwbc_plan::Row *dwbc_im_rows_l2(int *count);
extern "C" const dwbc_plan::Row *dwbc_im_rows_l3(int *count);
extern "C" const dwbc_plan::Row *dwbc_im_rows_l4(int *count);
extern "C" const dwbc_plan::Row *dwbc_im_rows_pair(int *count);
extern "C" const dwbc_plan::Row *dwbc_im_rows_lean(int *count);

// DWBC_F32 batches: the fp32 kernels (dwbc_kernels_f32.hip) work on the double buffers of the boundary; the model table is
// converted to float once
__global__ void dwbc_cvt_d2f(const double *__restrict__ in, float *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}

// part of [torque_grav_ | torque_task_ | torque_contact_] (sel 0..2) or their sum (sel 3), B x m
__global__ void dwbc_tau_select(const double *__restrict__ tau, double *__restrict__ out, int m, size_t cnt, int sel) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const size_t inst = i / m, j = i - inst * m;
    const double *s = tau + inst * 3 * m;
    out[i] = sel == 3 ? s[j] + s[m + j] + s[2 * m + j] : s[sel * m + j];
}

namespace dwbc {
std::string &capi_err() {
    static thread_local std::string e;
    return e;
}
}  // namespace dwbc
namespace {
int fail(const std::string &s) { return dwbc::capi_fail(s); }
}  // namespace
#define g_err (dwbc::capi_err())

extern "C" {

const char *dwbc_last_error(void) { return g_err.c_str(); }

int dwbc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

dwbc_model *dwbc_model_create_from_urdf(const char *path, int floating_base) {
    auto *mm = new dwbc_model();
    std::string err;
    if (!load_urdf(path, floating_base != 0, mm->m, err)) {
        g_err = err;
        delete mm;
        return nullptr;
    }
    return mm;
}

dwbc_model *dwbc_model_create_from_arrays(int nb, const int32_t *parent, const double *R_T, const double *p_T, const double *axis,
                                          const double *mass, const double *com, const double *inertia) {
    if (nb < 1 || nb > kMaxBodies) { g_err = "bad body count"; return nullptr; }
    auto *mm = new dwbc_model();
    Model &m = mm->m;
    m.parent.assign(parent, parent + nb);
    m.R_T.assign(R_T, R_T + 9 * nb);
    m.p_T.assign(p_T, p_T + 3 * nb);
    m.axis.assign(axis, axis + 3 * nb);
    m.mass.assign(mass, mass + nb);
    m.com.assign(com, com + 3 * nb);
    m.inertia.assign(inertia, inertia + 9 * nb);
    for (int i = 0; i < nb; i++) {
        m.names.push_back("link" + std::to_string(i));
        if (i > 0 && (parent[i] < 0 || parent[i] >= i)) { g_err = "parent[] must be a DFS pre-order"; delete mm; return nullptr; }
    }
    m.finalize();
    return mm;
}

void dwbc_model_destroy(dwbc_model *m) { delete m; }
int dwbc_model_num_links(const dwbc_model *m) { return m->m.nb; }
int dwbc_model_system_dof(const dwbc_model *m) { return m->m.ndof; }
double dwbc_model_total_mass(const dwbc_model *m) { return m->m.total_mass; }
int dwbc_model_link_id(const dwbc_model *m, const char *name) { return m->m.link_id(name); }
const char *dwbc_model_link_name(const dwbc_model *m, int link) {
    if (link == m->m.nb) return "COM";
    return (link >= 0 && link < m->m.nb) ? m->m.names[link].c_str() : "";
}
int dwbc_model_get_arrays(const dwbc_model *mm, int32_t *parent, double *R_T, double *p_T, double *axis, double *mass, double *com,
                          double *inertia) {
    const Model &m = mm->m;
    for (int i = 0; i < m.nb; i++) parent[i] = m.parent[i];
    memcpy(R_T, m.R_T.data(), sizeof(double) * 9 * m.nb);
    memcpy(p_T, m.p_T.data(), sizeof(double) * 3 * m.nb);
    memcpy(axis, m.axis.data(), sizeof(double) * 3 * m.nb);
    memcpy(mass, m.mass.data(), sizeof(double) * m.nb);
    memcpy(com, m.com.data(), sizeof(double) * 3 * m.nb);
    memcpy(inertia, m.inertia.data(), sizeof(double) * 9 * m.nb);
    return 1;
}

// ---- kernel packs: the cycle kernels of model sizes other than TOCABI's (dwbc_pack.hip), loaded on demand.  A pack is either
//      generic (any tree of its size) or built for one parent table (TopoPack: the tree-sparse sweep); the latter is preferred
//      when its table equals the model's
namespace {
struct KernelPack { void *dl; dwbc_plan::Table tab; std::vector<int> parents; };  // parents empty: generic
std::vector<KernelPack> g_packs;
std::mutex g_pack_mutex;
bool has_size(const dwbc_plan::Table &t, int n, int nb) {
    for (int i = 0; i < t.count; i++)
        if (t.rows[i].n == n && t.rows[i].nb == nb) return true;
    return false;
}
const dwbc_plan::Table kBuiltin{kRows, (int)(sizeof(kRows) / sizeof(kRows[0]))};
bool builtin_has(int n, int nb) { return has_size(kBuiltin, n, nb); }
// the rows of the per-instance-model build as one table (the planner takes the rows of a kind from one table)
dwbc_plan::Table inst_model_table() {
    static const std::vector<dwbc_plan::Row> rows = [] {
        std::vector<dwbc_plan::Row> v;
        for (const auto fn : {dwbc_im_rows_l1, dwbc_im_rows_l2, dwbc_im_rows_l3, dwbc_im_rows_l4, dwbc_im_rows_pair, dwbc_im_rows_lean}) {
            int n = 0;
            const dwbc_plan::Row *r = fn(&n);
            v.insert(v.end(), r, r + n);
        }
        return v;
    }();
    return dwbc_plan::Table{rows.data(), (int)rows.size()};
}
std::vector<int> clean_parents(const Model &m) {
    std::vector<int> p(m.parent.size());
    for (size_t i = 0; i < p.size(); i++) p[i] = m.parent[i] < 0 ? 0 : m.parent[i];
    return p;
}
unsigned tree_tag(const std::vector<int> &parents) {  // FNV-1a over the parents as little-endian 32-bit words (libdwbc_amd.build_pack names the file with it)
    unsigned h = 2166136261u;
    for (int p : parents)
        for (int b = 0; b < 4; b++) { h ^= (unsigned)((p >> (8 * b)) & 0xff); h *= 16777619u; }
    return h;
}
// the loaded pack of a model size built for exactly these parents (or, generic = true, for any tree); rows == nullptr: none
dwbc_plan::Table pack_lookup(int n, int nb, const std::vector<int> &parents, bool generic) {
    std::lock_guard<std::mutex> lk(g_pack_mutex);
    for (const auto &p : g_packs)
        if ((generic ? p.parents.empty() : p.parents == parents) && has_size(p.tab, n, nb)) return p.tab;
    return dwbc_plan::Table{nullptr, 0};
}
std::string lib_dir_impl() {
    Dl_info di;
    if (dladdr((const void *)&builtin_has, &di) && di.dli_fname) {
        std::string f(di.dli_fname);
        const size_t s = f.rfind('/');
        return s == std::string::npos ? std::string(".") : f.substr(0, s);
    }
    return ".";
}
// 1 loaded, 0 no such file, -1 unusable (err set)
int try_load_pack(const std::string &path, const std::vector<int> &parents, bool want_tree, std::string &err) {
    void *dl = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!dl) return 0;
    typedef const dwbc_plan::Row *(*table_fn)(int *, unsigned *);
    typedef const int *(*parents_fn)(int *);
    table_fn tf = (table_fn)dlsym(dl, "dwbc_pack_table");
    parents_fn pf = (parents_fn)dlsym(dl, "dwbc_pack_parents");
    int count = 0;
    unsigned tag = 0;
    const dwbc_plan::Row *tab = tf ? tf(&count, &tag) : nullptr;
    if (!tab || tag != kernel_abi_tag()) {
        dlclose(dl);
        err = path + " was built from another version of the kernels: rebuild it (make -C libdwbc_amd/csrc pack ...)";
        return -1;
    }
    KernelPack kp{dl, dwbc_plan::Table{tab, count}, {}};
    if (pf) {
        int pnb = 0;
        const int *pp = pf(&pnb);
        kp.parents.assign(pp, pp + pnb);
    }
    if (want_tree && kp.parents != parents) {  // a file with this tag but another tree (hash collision or a stale file): not ours
        dlclose(dl);
        return 0;
    }
    std::lock_guard<std::mutex> lk(g_pack_mutex);
    g_packs.push_back(kp);
    return 1;
}
// true when kernels for the model exist: built in, already loaded, or in a pack next to this library / under $DWBC_PACK_DIR
bool ensure_kernels(const Model &m, std::string &err) {
    const int n = m.ndof, nb = m.nb;
    if (builtin_has(n, nb)) return true;
    const std::vector<int> parents = clean_parents(m);
    if (pack_lookup(n, nb, parents, false).rows) return true;
    char tagbuf[16];
    snprintf(tagbuf, sizeof tagbuf, "%08x", tree_tag(parents));
    const std::string base = "libdwbc_pack_" + std::to_string(n) + "_" + std::to_string(nb);
    std::vector<std::string> dirs;
    if (const char *e = getenv("DWBC_PACK_DIR")) dirs.push_back(e);
    dirs.push_back(lib_dir_impl());
    std::string tried;
    for (const auto &d : dirs) {  // the pack of this very tree first
        const int r = try_load_pack(d + "/" + base + "_t" + tagbuf + ".so", parents, true, err);
        if (r < 0) return false;
        if (r > 0) return true;
    }
    if (pack_lookup(n, nb, parents, true).rows) return true;
    for (const auto &d : dirs) {
        const std::string path = d + "/" + base + ".so";
        const int r = try_load_pack(path, parents, false, err);
        if (r < 0) return false;
        if (r > 0) return true;
        tried += " " + path;
    }
    err = "no kernel for a model with " + std::to_string(n) + " dof / " + std::to_string(nb) + " bodies: the cycle kernels are compiled per model size; build the pack once with"
          " `make -C libdwbc_amd/csrc pack N=" + std::to_string(n) + " NB=" + std::to_string(nb) + "` (Python: libdwbc_amd.build_pack(model)); looked for" + tried;
    return false;
}
}  // namespace

// what the planner (dwbc_launch_plan.h) needs to know of a batch; the environment switches are read here and nowhere else
static dwbc_plan::Request plan_request(const dwbc_batch *b, bool reduced) {
    dwbc_plan::Request q{};
    q.n = b->n;
    q.nb = b->su.nb;
    q.levels = b->su.n_levels;
    q.topo = b->su.topo_kind;
    q.tree_match = b->tree_match;
    q.arith = b->dtype == DWBC_F32 ? dwbc_plan::kFloat : dwbc_plan::kDouble;
    q.B = b->B;
    q.n_cu = b->n_cu;
    q.reduced = reduced;
    q.max_active = b->max_active;
    q.n_contacts = b->su.n_contacts;
    q.wide_tasks = setup_wide_tasks(b->su);
    q.hqp = b->hqp != 0;
    q.warm = b->warm != 0;
    q.n_traj = b->su.n_traj;
    q.has_com_task = b->su.has_com_task != 0;
    q.n_custom = b->su.n_custom;
    q.dump_on = b->dump_on;
    q.inst_par = b->buf[dwbc_fields::kInstPar].d || !b->buf[dwbc_fields::kInstPar].h.empty();
    q.inst_model = b->buf[dwbc_fields::kInstModel].d || !b->buf[dwbc_fields::kInstModel].h.empty();
    q.no_wide = getenv("DWBC_NO_WIDE") != nullptr;
    q.no_pair = getenv("DWBC_NO_PAIR") != nullptr;
    q.no_lean = getenv("DWBC_NO_LEAN") != nullptr;
    q.pair_always = getenv("DWBC_PAIR_ALWAYS") != nullptr;
    // which wave of a two-wave workgroup is the main one can be swapped per workgroup (bit of the workgroup index) to steer the main
    // waves of a CU's four workgroups onto different SIMDs; measured at B = 1024 (profiles/r03e_pair_roles.txt): no swap 82.3 us per
    // launch, bit 8 / bit 9 99 - 102 us (the dispatcher already spreads wave 0 of consecutive workgroups), so the default is no swap
    const char *sb = getenv("DWBC_PAIR_SWAP_BIT");
    q.pair_swap_bit = sb ? atoi(sb) : -1;
    return q;
}

namespace fld = dwbc_fields;
using dwbc::Buf;

static dwbc_field_dims field_dims(const dwbc_batch *b) { return dwbc_field_dims{b->n, b->su.n_contacts, b->su.fstar_total, b->max_active}; }

int dwbc_field_describe(int index, const dwbc_field_dims *dims, dwbc_field_info *out) {
    if (index < 0 || index >= fld::kRowCount || !dims || !out) return 0;
    const fld::Row &r = fld::kRows[index];
    *out = fld::describe(r.id, r.name, r.type, r.shape, *dims, 0, (r.flags & fld::kBindable) != 0, (r.flags & fld::kMirror) != 0);
    return 1;
}

int dwbc_lean_output_describe(int family, int index, int n, int n_queried, dwbc_field_info *out) {
    if (family < 0 || family >= fld::kLeanCount || index < 0 || index >= fld::kLean[family].count || !out) return 0;
    const fld::LeanRow &r = fld::kLean[family].rows[index];
    *out = fld::describe(r.id, r.name, r.type, r.shape, dwbc_field_dims{n, 0, 0, 0}, n_queried, true, false);
    return 1;
}

size_t dwbc_batch_field_bytes(const dwbc_batch *b, int field) {
    const fld::Row *r = fld::find(field);
    return r ? (size_t)b->B * fld::elements(r->shape, field_dims(b)) * fld::item_size(r->type) : 0;
}

// ---- the buffer slots (dwbc_batch::buf).  The batch's device is current in all three.
static void release(Buf &u) {  // a bound buffer is let go of, an owned one freed
    if (u.own) (void)hipFree(u.d);
    u.d = nullptr; u.own = false; u.bytes = 0;
}
// an owned buffer of this size (a bound one stays: the caller sized it); a fresh one is marked for upload if the slot has a mirror
static int ensure(Buf &u, size_t bytes) {
    if (u.bound() || (u.d && u.bytes == bytes)) return 1;
    release(u);
    HIP_OK(hipMalloc(&u.d, bytes));
    u.own = true; u.bytes = bytes; u.dirty = !u.h.empty();
    return 1;
}
static int ensure_field(dwbc_batch *b, int field) { return ensure(b->buf[fld::find(field)->idx], dwbc_batch_field_bytes(b, field)); }
// the mirror of a slot to its own device buffer (sized like the mirror) if it is newer; *queued: a copy out of page-locked memory is in
// flight behind this (mark_upload)
static int send(dwbc_batch *b, int slot, bool *queued) {
    Buf &u = b->buf[slot];
    if (!u.h.empty() && !u.bound()) {
        if (!ensure(u, u.h.size())) return 0;
        if (u.dirty) {
            HIP_OK(hipMemcpyAsync(u.d, u.h.data(), u.h.size(), hipMemcpyHostToDevice, b->stream));
            *queued = *queued || u.h.pinned;
        }
    }
    u.dirty = false;
    return 1;
}
static int mark_upload(dwbc_batch *b) {
    if (!b->ev_upload) HIP_OK(hipEventCreateWithFlags(&b->ev_upload, hipEventDisableTiming));
    HIP_OK(hipEventRecord(b->ev_upload, b->stream));
    b->upload_pending = true;
    return 1;
}

static void wait_uploads(dwbc_batch *b);
// the per-instance parameter record, owned or bound, is let go of: the batch-wide values of the set-up hold again
static void drop_instance_params(dwbc_batch *b) {
    Buf &u = b->buf[fld::kInstPar];
    if (!u.d && u.h.empty()) return;
    hipSetDevice(b->device);
    wait_uploads(b);
    release(u);  // (hipFree waits for the launches that read it)
    u.h.clear();
    u.dirty = false;
}

// the per-instance body tables, owned or bound, are let go of: the model's own table holds for every instance again
static void drop_instance_model(dwbc_batch *b) {
    Buf &u = b->buf[fld::kInstModel];
    if (!u.d && u.h.empty()) return;
    hipSetDevice(b->device);
    wait_uploads(b);
    release(u);  // (hipFree waits for the launches that read it)
    u.h.clear();
    u.dirty = false;
}
// the body table a launch hands to its kernel: the per-instance record while the batch carries one (the planner then picks a dwbc_im::
// kernel, which reads table `inst` of it), else the model's
static const double *launch_body(const dwbc_batch *b) {
    const double *rec = b->dev<double>(fld::kInstModel);
    return rec ? rec : b->d_body;
}

// the task-space request and its outputs, owned or bound, are let go of: their shapes follow the task levels
static void drop_task_space(dwbc_batch *b) {
    if (!b->ts.mask) return;
    hipSetDevice(b->device);
    for (int s = fld::kTsFirst; s <= fld::kTsStatusSlot; s++) release(b->buf[s]);  // (hipFree waits for the launches that write them)
    b->ts.mask = 0;
    b->ts.ran = false;
}

// the single-level task-QP request, its outputs and its two inputs, owned or bound, are let go of: the level they name belongs to the task levels
static void drop_task_qp(dwbc_batch *b) {
    if (!b->tq.mask && !b->tq.prev_set && !b->tq.null_set) return;
    hipSetDevice(b->device);
    wait_uploads(b);
    for (int s = fld::kTqTorquePrev; s <= fld::kTqStatus; s++) {  // (hipFree waits for the launches that read and write them)
        release(b->buf[s]);
        b->buf[s].h.clear();
        b->buf[s].dirty = false;
    }
    b->tq = {};
}

dwbc_batch *dwbc_batch_create(const dwbc_model *m, int B, int device, int dtype) {
    if (!m || B < 1) { g_err = "bad arguments"; return nullptr; }
    if (dtype != DWBC_F64 && dtype != DWBC_F32) { g_err = "dtype must be DWBC_F64 or DWBC_F32"; return nullptr; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_err = "no HIP device: libdwbc_hip has no CPU path"; return nullptr; }
    if (device < 0 || device >= ndev) { g_err = "bad device index"; return nullptr; }
    if (m->m.ndof != m->m.nb + 5 || m->m.ndof > 50 || m->m.nb > kMaxBodies) {
        g_err = "model outside the kernels' range (floating base + one revolute joint per body, at most 50 dof)";
        return nullptr;
    }
    if (!ensure_kernels(m->m, g_err)) return nullptr;
    if (dtype == DWBC_F32 && !builtin_has(m->m.ndof, m->m.nb)) { g_err = "kernel packs are fp64 only"; return nullptr; }
    auto *b = new dwbc_batch();
    b->model = m;
    b->B = B;
    b->device = device;
    b->dtype = dtype;
    b->n = m->m.ndof;
    b->m = b->n - 6;
    b->tables[b->n_tables++] = kBuiltin;
    int n_f32 = 0;
    const dwbc_plan::Row *f32 = dwbc_f32_rows(&n_f32);
    b->tables[b->n_tables++] = dwbc_plan::Table{f32, n_f32};
    int n_ts = 0;
    const dwbc_plan::Row *ts = dwbc_task_space_rows(&n_ts);
    b->tables[b->n_tables++] = dwbc_plan::Table{ts, n_ts};
    int n_tq = 0;
    const dwbc_plan::Row *tq = dwbc_task_qp_rows(&n_tq);
    b->tables[b->n_tables++] = dwbc_plan::Table{tq, n_tq};
    b->tables[b->n_tables++] = inst_model_table();
    for (const bool generic : {false, true}) {
        const dwbc_plan::Table t = pack_lookup(b->n, m->m.nb, clean_parents(m->m), generic);
        if (!t.rows) continue;
        b->tables[b->n_tables++] = t;
        b->tree_match = b->tree_match || !generic;
    }
    b->dl = DumpLayout::make(b->n);
    setup_init(b->su, m->m.nb, b->n, m->m.maxdepth);
    auto bad = [&](const char *what, hipError_t e) {
        g_err = std::string(what) + ": " + hipGetErrorString(e);
        dwbc_batch_destroy(b);
        return (dwbc_batch *)nullptr;
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return bad("hipSetDevice", e);
    if ((e = hipDeviceGetAttribute(&b->n_cu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess) return bad("hipDeviceGetAttribute", e);
    std::vector<double> body;
    std::vector<int> topo;
    m->m.body_table(body);
    m->m.topo_table(topo);
    setup_set_parents(b->su, topo.data());
    if (getenv("DWBC_DENSE_SWEEP")) b->su.topo_kind = 0;  // test hook: the generic (dense) A^-1 sweep on a model that has a constant tree
    if ((e = hipMalloc(&b->d_body, body.size() * sizeof(double))) != hipSuccess) return bad("hipMalloc", e);
    if ((e = hipMalloc(&b->d_topo, topo.size() * sizeof(int))) != hipSuccess) return bad("hipMalloc", e);
    if ((e = hipMemcpy(b->d_body, body.data(), body.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return bad("hipMemcpy", e);
    if ((e = hipMemcpy(b->d_topo, topo.data(), topo.size() * sizeof(int), hipMemcpyHostToDevice)) != hipSuccess) return bad("hipMemcpy", e);
    for (const int f : {DWBC_IN_Q, DWBC_TAU, DWBC_WRENCH, DWBC_STATUS, DWBC_DIAG})
        if (!ensure_field(b, f)) { dwbc_batch_destroy(b); return nullptr; }
    hipMemset(b->buf[fld::kDiag].d, 0, b->buf[fld::kDiag].bytes);
    hipMemset(b->buf[fld::kStatus].d, 0, b->buf[fld::kStatus].bytes);
    b->buf[fld::kQ].h.assign(dwbc_batch_field_bytes(b, DWBC_IN_Q));
    b->buf[fld::kTauIn].h.assign(dwbc_batch_field_bytes(b, DWBC_IN_TORQUE));
    return b;
}

void dwbc_batch_destroy(dwbc_batch *b) {
    if (!b) return;
    hipSetDevice(b->device);
    for (Buf &u : b->buf) release(u);
    if (b->f_body) hipFree(b->f_body);
    hipFree(b->d_total);
    for (int l = 0; l < kMaxLevels; l++) hipFree(b->d_jacc[l]);
    hipFree(b->d_jacc_status);
    hipFree(b->d_rrec);
    hipFree(b->d_jacc_nc);
    hipFree(b->d_jacc_nc_status);
    hipFree(b->d_dump);
    hipFree(b->d_body);
    hipFree(b->d_topo);
    if (b->ev_upload) (void)hipEventDestroy(b->ev_upload);
    delete b;
}

int dwbc_batch_size(const dwbc_batch *b) { return b->B; }

int dwbc_batch_add_contact(dwbc_batch *b, int link, int contact_type, const double point[3], double lx, double ly, double mu,
                           double mu_z) {
    std::string err;
    const int i = setup_add_contact(b->su, link, contact_type, point, lx, ly, mu, mu_z, err);
    if (i < 0) { fail(err); return -1; }
    drop_instance_params(b);  // (its stride counts the contacts)
    b->buf[fld::kFlags].h.assign(dwbc_batch_field_bytes(b, DWBC_IN_CONTACT));
    b->buf[fld::kFlags].dirty = true;
    return i;
}

int dwbc_batch_clear_contacts(dwbc_batch *b) {
    b->su.n_contacts = 0;
    drop_instance_params(b);
    b->buf[fld::kFlags].h.clear();
    return 1;
}

int dwbc_batch_add_task(dwbc_batch *b, int level, int mode, int link, const double point[3]) {
    std::string err;
    if (!setup_add_task(b->su, level, mode, link, point, err)) return fail(err);
    drop_task_space(b);
    drop_task_qp(b);
    b->buf[fld::kFstar].h.assign(dwbc_batch_field_bytes(b, DWBC_IN_FSTAR));
    b->buf[fld::kFstar].dirty = true;
    return 1;
}

int dwbc_batch_add_custom_task(dwbc_batch *b, int level, int task_dof) {
    std::string err;
    if (!setup_add_custom_task(b->su, level, task_dof, err)) return fail(err);
    drop_task_space(b);
    drop_task_qp(b);
    b->buf[fld::kFstar].h.assign(dwbc_batch_field_bytes(b, DWBC_IN_FSTAR));
    b->buf[fld::kFstar].dirty = true;
    b->buf[fld::kCustom].h.assign((size_t)b->B * b->su.n_custom * kMaxTaskDof * b->n * sizeof(double));
    b->buf[fld::kCustom].dirty = true;
    return 1;
}

int dwbc_batch_set_custom_task(dwbc_batch *b, int level, const double *fstar, const double *J) {
    if (level < 0 || level >= b->su.n_levels) return fail("ERROR : task space size overflow");
    const int slot = b->su.t_custom_slot[level];
    if (slot < 0) return fail("not a TASK_CUSTOM level");
    if (!J) return fail("J_task is NULL");
    if (fstar && !dwbc_batch_set_fstar(b, level, fstar)) return 0;
    const int t = b->su.t_dof[level], n = b->n, ns = b->su.n_custom;
    const size_t stride = (size_t)kMaxTaskDof * n;
    double *hc = b->buf[fld::kCustom].h.as<double>();
    for (int i = 0; i < b->B; i++) memcpy(hc + ((size_t)i * ns + slot) * stride, J + (size_t)i * t * n, sizeof(double) * t * n);
    b->buf[fld::kCustom].dirty = true;
    return 1;
}

int dwbc_batch_clear_tasks(dwbc_batch *b) {
    drop_task_space(b);
    drop_task_qp(b);
    b->su.n_levels = 0;
    b->su.has_com_task = 0;
    b->su.n_custom = 0;
    for (int l = 0; l < kMaxLevels; l++) b->su.t_custom_slot[l] = -1;
    b->buf[fld::kCustom].h.clear();
    setup_fstar_layout(b->su);
    b->buf[fld::kFstar].h.clear();
    b->su.n_traj = 0;
    for (int l = 0; l < kMaxLevels; l++)
        for (int j = 0; j < kMaxTaskLinks; j++) b->su.t_traj_slot[l][j] = -1;
    b->buf[fld::kTraj].h.clear();
    return 1;
}

int dwbc_batch_set_task_gain(dwbc_batch *b, int level, int link_index, const double *pos_p, const double *pos_d, const double *pos_a,
                             const double *rot_p, const double *rot_d, const double *rot_a) {
    if (level < 0 || level >= b->su.n_levels || link_index < 0 || link_index >= b->su.t_nlinks[level]) return fail("bad task level / link index");
    (void)rot_a;  // stored by the reference, never read by GetFstarRotPD (src/task.cpp:338)
    double *g = b->su.t_gain[level][link_index];
    for (int a = 0; a < 3; a++) { g[a] = pos_p[a]; g[3 + a] = pos_d[a]; g[6 + a] = pos_a[a]; g[9 + a] = rot_p[a]; g[12 + a] = rot_d[a]; }
    return 1;
}

int dwbc_batch_set_trajectory(dwbc_batch *b, int level, int link_index, const double *traj) {
    if (level < 0 || level >= b->su.n_levels || link_index < 0 || link_index >= b->su.t_nlinks[level]) return fail("bad task level / link index");
    int &slot = b->su.t_traj_slot[level][link_index];
    HostBytes &ht = b->buf[fld::kTraj].h;
    if (!traj) {  // back to SetTaskSpace values for this link (slots of other links keep their place)
        slot = -1;
        return 1;
    }
    if (slot < 0) {
        if (b->su.n_traj >= kMaxLevels * kMaxTaskLinks) return fail("too many trajectories");
        // records are instance-major: re-stride the host copy for the new slot count
        const int old = b->su.n_traj, now = old + 1;
        std::vector<double> h((size_t)b->B * now * kTrajStride, 0.0);
        for (int i = 0; i < b->B; i++)
            for (int sidx = 0; sidx < old; sidx++)
                memcpy(&h[((size_t)i * now + sidx) * kTrajStride], ht.as<double>() + ((size_t)i * old + sidx) * kTrajStride, kTrajStride * sizeof(double));
        ht.assign(h.data(), h.size() * sizeof(double));
        slot = old;
        b->su.n_traj = now;
    }
    const int ns = b->su.n_traj;
    for (int i = 0; i < b->B; i++)
        memcpy(ht.as<double>() + ((size_t)i * ns + slot) * kTrajStride, traj + (size_t)i * kTrajStride, kTrajStride * sizeof(double));
    b->buf[fld::kTraj].dirty = true;
    return 1;
}

int dwbc_batch_set_control_time(dwbc_batch *b, const double *t) {
    if (!t) return fail("control time is NULL");
    b->buf[fld::kCtime].h.assign(t, (size_t)b->B * sizeof(double));
    b->buf[fld::kCtime].dirty = true;
    return 1;
}

int dwbc_batch_set_torque_limit(dwbc_batch *b, const double *tau_lim) {
    if (!tau_lim) { b->su.has_tau_lim = 0; return 1; }
    b->su.has_tau_lim = 1;
    for (int i = 0; i < b->m; i++) b->su.tau_lim[i] = tau_lim[i];
    return 1;
}

int dwbc_batch_instance_param_stride(const dwbc_batch *b) { return b->m + 4 * b->su.n_contacts; }

int dwbc_batch_set_instance_params(dwbc_batch *b, const double *host) {
    Buf &u = b->buf[fld::kInstPar];
    if (u.bound()) return fail("the instance parameters are bound to a device buffer");
    if (!host) { drop_instance_params(b); return 1; }
    if (b->su.n_contacts < 1) return fail("instance parameters: register the contacts first (the record holds four constants per contact)");
    const size_t cnt = (size_t)b->B * dwbc_batch_instance_param_stride(b);
    for (size_t i = 0; i < cnt; i++)
        if (!std::isfinite(host[i]) || !(host[i] > 0.0)) return fail("instance parameters: every torque limit and contact constant must be finite and > 0");
    wait_uploads(b);
    u.h.assign(host, cnt * sizeof(double));
    u.dirty = true;
    return 1;
}

int dwbc_batch_bind_instance_params(dwbc_batch *b, void *p) {
    Buf &u = b->buf[fld::kInstPar];
    if (!p && !u.bound()) return 1;  // nothing bound
    drop_instance_params(b);
    u.d = p;
    return 1;
}

// ---- one body table per instance (mass, COM, inertia and joint frames): B x nb x kBodyStride doubles in the layout of Model::body_table
int dwbc_batch_instance_model_stride(const dwbc_batch *b) { return b->su.nb * kBodyStride; }

// why this batch cannot carry a record at all (nullptr: it can)
static const char *instance_model_refusal(const dwbc_batch *b) {
    if (b->dtype == DWBC_F32) return "per-instance model: fp64 batches only";
    if (!builtin_has(b->n, b->su.nb)) return "per-instance model: not built for kernel-pack models (TOCABI's size and tree only)";
    if (b->su.topo_kind != 1) return "per-instance model: built for TOCABI's constant tree only (this model's tree differs, or the batch was created under DWBC_DENSE_SWEEP)";
    return nullptr;
}

int dwbc_batch_set_instance_model(dwbc_batch *b, const double *host) {
    Buf &u = b->buf[fld::kInstModel];
    if (const char *why = instance_model_refusal(b)) return fail(why);
    if (u.bound()) return fail("the instance model is bound to a device buffer");
    if (!host) { drop_instance_model(b); return 1; }
    const int nb = b->su.nb;
    for (int i = 0; i < b->B; i++)
        for (int k = 0; k < nb; k++) {
            const double *r = host + ((size_t)i * nb + k) * kBodyStride;
            auto bad = [&](const char *what) { return fail("instance model: instance " + std::to_string(i) + ", body " + std::to_string(k) + ": " + what); };
            for (int a = 0; a < kBodyStride; a++)
                if (!std::isfinite(r[a])) return bad("an entry is not finite");
            if (!(r[BF_MASS] > 0.0)) return bad("mass must be > 0");
            if (!(r[BF_ICOM] > 0.0) || !(r[BF_ICOM + 3] > 0.0) || !(r[BF_ICOM + 5] > 0.0)) return bad("the diagonal of the inertia must be > 0");
            if (k == 0) continue;  // (the floating base has no joint)
            const double *ax = r + BF_AXIS, *R = r + BF_RT;
            if (std::fabs(std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) - 1.0) > 1e-6) return bad("the joint axis must have unit length (to 1e-6)");
            for (int x = 0; x < 3; x++)
                for (int y = 0; y < 3; y++) {
                    const double d = R[3 * x] * R[3 * y] + R[3 * x + 1] * R[3 * y + 1] + R[3 * x + 2] * R[3 * y + 2];
                    if (std::fabs(d - (x == y ? 1.0 : 0.0)) > 1e-6) return bad("R_T must be orthonormal (R_T R_T^T = I to 1e-6)");
                }
        }
    wait_uploads(b);
    u.h.assign(host, (size_t)b->B * nb * kBodyStride * sizeof(double));
    u.dirty = true;
    return 1;
}

int dwbc_batch_bind_instance_model(dwbc_batch *b, void *p) {
    Buf &u = b->buf[fld::kInstModel];
    if (const char *why = instance_model_refusal(b)) return fail(why);
    if (!p && !u.bound()) return 1;  // nothing bound
    drop_instance_model(b);
    u.d = p;
    return 1;
}

int dwbc_batch_fstar_size(const dwbc_batch *b) { return b->su.fstar_total; }
int dwbc_batch_task_dof(const dwbc_batch *b, int level) { return (level >= 0 && level < b->su.n_levels) ? b->su.t_dof[level] : 0; }

// An upload of the page-locked mirrors may still be in flight (hipMemcpyAsync returns at once): wait for it before a mirror is
// rewritten, so that a pipelined `solve(); set_state(next); solve();` never tears the inputs of the first solve.
static void wait_uploads(dwbc_batch *b) {
    if (!b->upload_pending) return;
    if (b->ev_upload) (void)hipEventSynchronize(b->ev_upload);
    b->upload_pending = false;
}

int dwbc_batch_set_state(dwbc_batch *b, const double *q, const double *qdot, const double *qddot) {
    (void)qddot;  // the reference hands it to RBDL's UpdateKinematicsCustom only; nothing on this path reads accelerations
    if (!q) return fail("q is NULL");
    Buf &uq = b->buf[fld::kQ];
    if (uq.bound()) return fail("q is bound to a device buffer");
    wait_uploads(b);
    if (q != uq.h.as<double>()) memcpy(uq.h.data(), q, uq.h.size());  // (dwbc_batch_host_ptr: already in place)
    uq.dirty = true;
    if (qdot) {  // B_, link velocities (dump record) and the on-device task reference need it; the torque path does not
        b->buf[fld::kQdot].h.assign(qdot, (size_t)b->B * b->n * sizeof(double));
        b->buf[fld::kQdot].dirty = true;
    }
    return 1;
}

int dwbc_batch_set_contact(dwbc_batch *b, const uint8_t *flags) {
    if (b->su.n_contacts == 0) return fail("Contact Constraint size mismatch");  // include/dwbc.h:438-441
    Buf &uf = b->buf[fld::kFlags];
    if (uf.bound()) return fail("contact flags are bound to a device buffer");
    // the product kernels stack two simultaneous 6D contacts, the general-contact kernel three (the reference: any number,
    // src/dwbc.cpp:445-453); an instance with more than the batch is set up for is refused here instead of failing on the device
    const int ncn = b->su.n_contacts;
    for (int i = 0; i < b->B; i++) {
        int on = 0;
        for (int c = 0; c < ncn; c++) on += flags[(size_t)i * ncn + c] ? 1 : 0;
        if (on > b->max_active)
            return fail(b->max_active > 2 ? "more than 3 simultaneously active contacts in one instance: not supported by the device path"
                                          : "more than 2 simultaneously active contacts in one instance: call dwbc_batch_set_max_active_contacts(b, 3) first (3 is the most the device path stacks)");
    }
    wait_uploads(b);
    if (flags != uf.h.data()) memcpy(uf.h.data(), flags, uf.h.size());
    uf.dirty = true;
    return 1;
}

// SetContact with more than two flags raised (reference src/dwbc.cpp:445-453 stacks every flagged contact): n = 3 routes the
// batch's solves through the general-contact kernel (dwbc_cycle_gc.h) and widens the wrench output to 6 n doubles per instance
int dwbc_batch_set_max_active_contacts(dwbc_batch *b, int n) {
    if (n != 2 && n != kGcContacts) return fail("max active contacts: 2 (default) or 3");
    if (n == b->max_active) return 1;
    if (n > 2) {
        if (b->dtype == DWBC_F32) return fail("three active contacts: fp64 batches only");
        const dwbc_plan::Request q = plan_request(b, false);
        if (q.inst_model) return fail(dwbc_plan::kInstModelGc);
        if (!dwbc_plan::Candidates(q, dwbc_plan::kGc, b->tables, b->n_tables).pick(dwbc_plan::kWideTasks, 0u)) return fail("no general-contact kernel for this model size (built in for TOCABI; kernel packs carry one for models of at most 40 dof)");
    }
    Buf &uw = b->buf[fld::kWrench];
    if (uw.bound()) return fail("wrench is bound to a device buffer: set the contact capacity before binding");
    if (n < b->max_active) {  // lowering the capacity: the flags already set must fit it (they were validated against the old one)
        const int ncn = b->su.n_contacts;
        const HostBytes &hf = b->buf[fld::kFlags].h;
        for (int i = 0; i < b->B && ncn > 0 && !hf.empty(); i++) {
            int on = 0;
            for (int c = 0; c < ncn; c++) on += hf[(size_t)i * ncn + c] ? 1 : 0;
            if (on > n) return fail("max active contacts: the contact flags of this batch hold an instance with more active contacts than the new capacity");
        }
    }
    HIP_OK(hipSetDevice(b->device));  // (the new buffer must live on the batch's device whatever device is current in the caller's thread)
    HIP_OK(hipStreamSynchronize(b->stream));
    // the new buffer first, the swap only on success: a failed allocation leaves the batch as it was
    dwbc_field_dims dims = field_dims(b);
    dims.max_active = n;
    const size_t bytes = (size_t)b->B * fld::elements(fld::find(DWBC_WRENCH)->shape, dims) * sizeof(double);
    void *nw = nullptr;
    HIP_OK(hipMalloc(&nw, bytes));
    if (hipMemset(nw, 0, bytes) != hipSuccess) {
        (void)hipFree(nw);
        return fail("max active contacts: hipMemset of the new wrench buffer failed");
    }
    release(uw);
    uw.d = nw; uw.own = true; uw.bytes = bytes;
    b->max_active = n;
    return 1;
}
int dwbc_batch_max_active_contacts(const dwbc_batch *b) { return b->max_active; }

int dwbc_batch_set_fstar(dwbc_batch *b, int level, const double *fstar) {
    if (level < 0 || level >= b->su.n_levels) return fail("ERROR : task space size overflow");  // src/dwbc.cpp:668-671
    Buf &uf = b->buf[fld::kFstar];
    if (uf.bound()) return fail("f* is bound to a device buffer");
    const int t = b->su.t_dof[level], off = b->su.fstar_off[level], F = b->su.fstar_total;
    wait_uploads(b);
    double *hf = uf.h.as<double>();
    if (fstar != hf + off)  // (a caller that filled the mirror in place passes host_ptr + off)
        for (int i = 0; i < b->B; i++) memcpy(hf + (size_t)i * F + off, fstar + (size_t)i * t, sizeof(double) * t);
    uf.dirty = true;
    return 1;
}

void *dwbc_batch_host_ptr(dwbc_batch *b, int field) {
    wait_uploads(b);  // the caller is about to write into the mirror
    const fld::Row *r = fld::find(field);
    if (!r || !(r->flags & fld::kMirror)) return nullptr;
    return b->buf[r->idx].h.data();  // (NULL while the field has no size)
}

int dwbc_batch_bind_device(dwbc_batch *b, int field, void *p) {
    if (!p) return fail("NULL device pointer");
    hipSetDevice(b->device);
    const fld::Row *r = fld::find(field);
    if (!r || !(r->flags & fld::kBindable)) return fail("field cannot be bound");
    Buf &u = b->buf[r->idx];
    release(u);
    u.d = p; u.dirty = false;
    if (field == DWBC_IN_TORQUE) b->tau_in_set = true;
    return 1;
}

int dwbc_batch_set_stream(dwbc_batch *b, void *s) { b->stream = (hipStream_t)s; return 1; }

int dwbc_batch_enable_dump(dwbc_batch *b, int on) {
    hipSetDevice(b->device);
    if (on && !b->d_dump) HIP_OK(hipMalloc(&b->d_dump, (size_t)b->B * b->dl.total * sizeof(double)));
    b->dump_on = on != 0;
    return 1;
}

// the mirrors of these slots that are newer than their device buffers, in this order; every launch reads the model, so the per-instance
// body tables go first whatever the slots are
static int send_inputs(dwbc_batch *b, std::initializer_list<int> slots) {
    bool queued = false;
    if (!send(b, fld::kInstModel, &queued)) return 0;
    for (const int slot : slots)
        if (!send(b, slot, &queued)) return 0;
    return queued ? mark_upload(b) : 1;
}
static int upload_inputs(dwbc_batch *b) {  // what the cycle reads
    return send_inputs(b, {fld::kTraj, fld::kCustom, fld::kCtime, fld::kInstPar, fld::kQdot, fld::kQ, fld::kFlags, fld::kFstar});
}

// the set-up a launch hands to the kernel: with a per-instance parameter record the torque rows exist as after dwbc_batch_set_torque_limit
static const Setup *launch_setup(const dwbc_batch *b, const BatchIO &io, Setup &tmp) {
    if (!io.inst_par || b->su.has_tau_lim) return &b->su;
    tmp = b->su;
    tmp.has_tau_lim = 1;
    return &tmp;
}

// the kernel of an accepted plan on the batch's stream, one workgroup per instance; its dynamic-LDS attribute is raised once per kernel
// and batch
static int launch_kernel(dwbc_batch *b, const dwbc_plan::Plan &p, void **args) {
    const void *fn = p.row->fn;
    if (std::find(b->lds_attr_set.begin(), b->lds_attr_set.end(), fn) == b->lds_attr_set.end()) {
        HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds));
        b->lds_attr_set.push_back(fn);
    }
    HIP_OK(hipLaunchKernel(fn, dim3(b->B), dim3(p.threads), args, p.lds, b->stream));
    return 1;
}

// one launch of the cycle: the planner picks the build, whatever its arithmetic type or kind
static int launch(dwbc_batch *b, bool reduced) {
    const dwbc_plan::Plan p = dwbc_plan::plan(plan_request(b, reduced), b->tables, b->n_tables);
    if (!p.row) return fail(p.err);
    // the fp32 kernels read and write the double buffers of the boundary themselves (io_t); only the model table is kept in float
    const bool f32 = b->dtype == DWBC_F32;
    if (f32 && !b->f_body) {
        std::vector<double> body;
        b->model->m.body_table(body);
        HIP_OK(hipMalloc(&b->f_body, body.size() * sizeof(float)));
        hipLaunchKernelGGL(dwbc_cvt_d2f, dim3((unsigned)((body.size() + 255) / 256)), dim3(256), 0, b->stream, b->d_body, b->f_body, body.size());
    }
    BatchIO io{};
    io.B = b->B;
    io.q = b->dev<double>(fld::kQ);
    io.qdot = b->dev<double>(fld::kQdot);
    io.traj = b->su.n_traj > 0 ? b->dev<double>(fld::kTraj) : nullptr;
    io.ctime = b->dev<double>(fld::kCtime);
    io.custom_J = b->su.n_custom > 0 ? b->dev<double>(fld::kCustom) : nullptr;
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.fstar = b->dev<double>(fld::kFstar);
    io.tau = b->dev<double>(fld::kTau);
    io.wrench = b->dev<double>(fld::kWrench);
    io.wrench_ld = 6 * b->max_active;
    io.status = b->dev<int>(fld::kStatus);
    io.diag = b->dev<int>(fld::kDiag);
    io.dump = b->dump_on ? b->d_dump : nullptr;  // (never on an fp32 batch: the planner refuses it)
    io.body = f32 ? reinterpret_cast<const double *>(b->f_body) : launch_body(b);  // real_t of the build that p.row belongs to
    io.topo = b->d_topo;
    io.hqp = b->hqp;
    io.pair_swap_bit = p.pair_swap_bit;
    io.warm = (b->warm && b->ws_valid) ? 1 : 0;
    io.inst_par = b->dev<double>(fld::kInstPar);
    Setup su_rec;
    void *args[] = {(void *)launch_setup(b, io, su_rec), (void *)&io};
    if (!launch_kernel(b, p, args)) return 0;
    b->ws_valid = p.ws_valid_after;
    b->last = p;
    return 1;
}

int dwbc_batch_solve(dwbc_batch *b, unsigned flags) {
    b->hqp = (flags & DWBC_SOLVE_HQP) ? 1 : 0;
    // init = false (DWBC_SOLVE_INIT clear): hot start from the working sets of the previous solve (src/dwbc.cpp:1064-1074).  The
    // first solve of a batch, and the first after the lean kernel ran, has no working set to start from and runs cold.
    b->warm = (flags & DWBC_SOLVE_INIT) ? 0 : 1;
    if (!b->hqp && (flags & DWBC_SOLVE_REDUCED)) return fail("hqp=false is not built on the reduced dynamics path");
    if (b->su.n_levels < 1) return fail("no task space");
    if (b->su.n_contacts < 1) return fail("no contact constraint");
    const bool reduced = flags & DWBC_SOLVE_REDUCED;
    b->last_reduced = reduced;
    if (reduced && b->su.n_custom > 0) return fail("TASK_CUSTOM levels are not built on the reduced dynamics path");
    if (reduced && b->su.has_tau_lim)
        return fail("reduced dynamics path with a torque limit is inconsistent in the reference (src/dwbc.cpp:3462-3467,3513; "
                    "its harness disables the limit, tests/sp_test/redu_dyn_test.cpp:63): call dwbc_batch_set_torque_limit(b, NULL)");
    HIP_OK(hipSetDevice(b->device));
    if (!upload_inputs(b)) return 0;
    return launch(b, reduced);
}

// ---- CalcContactRedistribute(torque_input, hqp, init) on a caller-supplied torque: the lean kernel of dwbc_redistribute.h
int dwbc_batch_set_torque_input(dwbc_batch *b, const double *tau) {
    if (!tau) return fail("torque input is NULL");
    Buf &u = b->buf[fld::kTauIn];
    if (u.bound()) return fail("the torque input is bound to a device buffer");
    wait_uploads(b);
    if (tau != u.h.as<double>()) memcpy(u.h.data(), tau, u.h.size());  // (dwbc_batch_host_ptr: already in place)
    u.dirty = true;
    b->tau_in_set = true;
    return 1;
}

// the planner's view of a redistribution on this batch: the model, the arithmetic type and the contact capacity of the batch, hqp of
// the call (the cycle's own hqp / warm state is neither read nor changed)
static dwbc_plan::Plan redist_plan(const dwbc_batch *b, bool hqp) {
    dwbc_plan::Request q = plan_request(b, false);
    q.redistribute = true;
    q.hqp = hqp;
    return dwbc_plan::plan(q, b->tables, b->n_tables);
}

// ---- what the lean launches share (enum dwbc_lean_family; their outputs: dwbc_fields::kLean).  Per family there remain the kernel's IO
// records, the inputs it uploads and its preconditions
static dwbc_plan::Plan lean_plan(const dwbc_batch *b, int family) {
    static constexpr bool dwbc_plan::Request::*kind[] = {&dwbc_plan::Request::grav_comp, &dwbc_plan::Request::link_query, &dwbc_plan::Request::dynamics,
                                                         &dwbc_plan::Request::contact_space};
    dwbc_plan::Request q = plan_request(b, false);
    q.*kind[family] = true;
    return dwbc_plan::plan(q, b->tables, b->n_tables);
}

// name of a plan's kernel as rocprofv3 prints the instantiation, "" with the error set for a refused one; a string per family (and one, at
// the end, for the redistribution) and thread
static const char *plan_name(const dwbc_plan::Plan &p, int which) {
    static thread_local char name[fld::kLeanCount + 1][160];
    if (!p.row) { fail(p.err); return ""; }
    dwbc_plan::format_name(*p.row, name[which], sizeof name[which]);
    return name[which];
}

// bytes of all B instances of one output under the family's request (0: not part of it, no such output)
static size_t lean_bytes(const dwbc_batch *b, int family, int what) {
    const fld::Family &f = fld::kLean[family];
    if (what < 0 || what >= f.count || !((b->lean[family].mask >> what) & 1u)) return 0;
    return (size_t)b->B * fld::elements(f.rows[what].shape, field_dims(b), b->lq_n) * fld::item_size(f.rows[what].type);
}

// why output `what` of the family cannot be named (nullptr: it can)
static const char *lean_refusal(const dwbc_batch *b, int family, int what) {
    const fld::Family &f = fld::kLean[family];
    if (what < 0 || what >= f.count) return f.unknown;
    if (!b->lean[family].mask) return f.no_request;
    if (!((b->lean[family].mask >> what) & 1u)) return f.not_asked;
    return nullptr;
}

static int read_back(dwbc_batch *b, const void *src, void *out, size_t nbytes);
static int lean_get(dwbc_batch *b, int family, int what, void *out, size_t bytes) {
    if (const char *why = lean_refusal(b, family, what)) return fail(why);
    if (!b->lean[family].ran) return fail(fld::kLean[family].not_run);
    const size_t need = lean_bytes(b, family, what);
    if (bytes < need) return fail("output buffer too small");
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    return read_back(b, b->buf[fld::kLean[family].rows[what].slot].d, out, need);
}

static int lean_bind(dwbc_batch *b, int family, int what, void *p) {
    if (const char *why = lean_refusal(b, family, what)) return fail(why);
    HIP_OK(hipSetDevice(b->device));
    Buf &u = b->buf[fld::kLean[family].rows[what].slot];
    release(u);
    b->lean[family].ran = false;  // (what the batch's own buffer held is not in the new one)
    if (!p) return ensure(u, lean_bytes(b, family, what));
    u.d = p;
    return 1;
}

// the outputs of the family's request exist (bound ones stay bound)
static int lean_ensure(dwbc_batch *b, int family) {
    for (int w = 0; w < fld::kLean[family].count; w++)
        if (const size_t bytes = lean_bytes(b, family, w))
            if (!ensure(b->buf[fld::kLean[family].rows[w].slot], bytes)) return 0;
    return 1;
}

// a new request: outputs of the new sizes, owned by the batch (a buffer bound for the old request may be too small for the new one);
// allocated here, so that the launch itself allocates nothing
static int lean_request(dwbc_batch *b, int family, unsigned mask) {
    HIP_OK(hipSetDevice(b->device));
    for (int w = 0; w < fld::kLean[family].count; w++) release(b->buf[fld::kLean[family].rows[w].slot]);  // (hipFree waits for the launches that write them)
    b->lean[family].mask = mask;
    b->lean[family].ran = false;
    return lean_ensure(b, family);
}

// dwbc_batch_set_*_outputs: a refused mask leaves the request and the outputs of the batch as they were
static int lean_set_outputs(dwbc_batch *b, int family, unsigned mask) {
    const fld::Family &f = fld::kLean[family];
    if (mask & ~f.all()) return fail(f.unknown_bit);
    if (mask) {
        const dwbc_plan::Plan p = lean_plan(b, family);
        if (!p.row) return fail(p.err);
        mask |= 1u << f.status;
    }
    return lean_request(b, family, mask);
}

// what every lean kernel reads: the state and the model
static BatchIO lean_io(const dwbc_batch *b) {
    BatchIO io{};
    io.B = b->B;
    io.q = b->dev<double>(fld::kQ);
    io.body = launch_body(b);
    io.topo = b->d_topo;
    io.pair_swap_bit = -1;
    return io;
}

// dwbc_batch_time_*: first() -- uploads and one warm launch -- then K launches by again(), bracketed by HIP events on the batch's stream;
// the events are destroyed on every way out (a failed step has set the error string)
extern "C++" {
template <class First, class Again>
static int time_launches(dwbc_batch *b, int steps, float *ms, First first, Again again) {
    HIP_OK(hipSetDevice(b->device));
    if (!first()) return 0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto timed = [&]() -> int {
        HIP_OK(hipEventCreate(&e0));
        HIP_OK(hipEventCreate(&e1));
        HIP_OK(hipEventRecord(e0, b->stream));
        for (int i = 0; i < steps; i++)
            if (!again()) return 0;
        HIP_OK(hipEventRecord(e1, b->stream));
        HIP_OK(hipEventSynchronize(e1));
        HIP_OK(hipEventElapsedTime(ms, e0, e1));
        return 1;
    };
    const int ok = timed();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ok;
}
}

int dwbc_batch_time_solves(dwbc_batch *b, unsigned flags, int steps, float *ms) {
    return time_launches(b, steps, ms, [&] { return dwbc_batch_solve(b, flags); }, [&] { return launch(b, flags & DWBC_SOLVE_REDUCED); });
}

static int launch_redistribute(dwbc_batch *b, const dwbc_plan::Plan &p) {
    BatchIO io = lean_io(b);  // what stage 0 and the contact stage read; no output of the cycle is named
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.fstar = b->dev<double>(fld::kFstar);
    io.hqp = 1;
    io.inst_par = b->dev<double>(fld::kInstPar);
    Setup su_rec;
    RedistIO rio{b->dev<double>(fld::kTauIn), b->dev<double>(fld::kRdTau), b->dev<double>(fld::kRdCf), b->dev<double>(fld::kRdWrench), b->dev<int>(fld::kRdStatus)};
    void *args[] = {(void *)launch_setup(b, io, su_rec), (void *)&io, (void *)&rio};
    return launch_kernel(b, p, args);
}

// ---- CalcGravCompensation on its own, or ahead of the redistribution of a command on top of it: dwbc_redistribute.h with GRAV = true
// with_input: the redistribution of torque_grav_ + torque input goes with it
static int launch_grav(dwbc_batch *b, const dwbc_plan::Plan &p, bool with_input) {
    BatchIO io = lean_io(b);  // what stage 0 and the contact stage read; no buffer of the cycle or of the link query is named
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.fstar = b->dev<double>(fld::kFstar);
    io.hqp = 1;
    io.inst_par = with_input ? b->dev<double>(fld::kInstPar) : nullptr;  // (QP rows alone read the record)
    Setup su_rec;
    GravIO gio{};
    if (with_input) {
        gio.tau_in = b->dev<double>(fld::kTauIn);
        gio.rd_tau = b->dev<double>(fld::kRdTau);
        gio.rd_cf = b->dev<double>(fld::kRdCf);
        gio.rd_wrench = b->dev<double>(fld::kRdWrench);
        gio.rd_status = b->dev<int>(fld::kRdStatus);
    }
    gio.tau = b->dev<double>(fld::kGvTau);
    gio.wrench = b->dev<double>(fld::kGvWrench);
    gio.status = b->dev<int>(fld::kGvStatus);
    void *args[] = {(void *)launch_setup(b, io, su_rec), (void *)&io, (void *)&gio};
    if (!launch_kernel(b, p, args)) return 0;
    b->lean[DWBC_LEAN_GRAV].ran = true;
    return 1;
}

// uploads whatever is pending, launches once; *planned (optional): the plan of the launch, for a caller that repeats it
static int grav_once(dwbc_batch *b, dwbc_plan::Plan *planned) {
    const dwbc_plan::Plan p = lean_plan(b, DWBC_LEAN_GRAV);
    if (!p.row) return fail(p.err);
    if (b->su.n_contacts < 1) return fail("no contact constraint");
    HIP_OK(hipSetDevice(b->device));
    if (!upload_inputs(b)) return 0;  // (the state and the flags are read; stage 0 stages f* of a batch that has task levels)
    if (!lean_ensure(b, DWBC_LEAN_GRAV)) return 0;  // (the one family whose outputs are not allocated by a request)
    if (planned) *planned = p;
    return launch_grav(b, p, false);
}

int dwbc_batch_grav_compensation(dwbc_batch *b) { return grav_once(b, nullptr); }
int dwbc_batch_time_grav(dwbc_batch *b, int steps, float *ms) {
    dwbc_plan::Plan p{};
    return time_launches(b, steps, ms, [&] { return grav_once(b, &p); }, [&] { return launch_grav(b, p, false); });
}
size_t dwbc_batch_grav_bytes(const dwbc_batch *b, int what) { return lean_bytes(b, DWBC_LEAN_GRAV, what); }
int dwbc_batch_get_grav(dwbc_batch *b, int what, void *out, size_t bytes) { return lean_get(b, DWBC_LEAN_GRAV, what, out, bytes); }
int dwbc_batch_bind_grav(dwbc_batch *b, int what, void *p) { return lean_bind(b, DWBC_LEAN_GRAV, what, p); }
const char *dwbc_batch_grav_kernel_name(const dwbc_batch *b) { return plan_name(lean_plan(b, DWBC_LEAN_GRAV), DWBC_LEAN_GRAV); }

// uploads whatever is pending, launches once; *planned (optional): the plan of the launch, for a caller that repeats it
// DWBC_REDIST_ADD_GRAVITY: every refusal of the plain redistribution first, then the gravity-compensation kernel in its place
static int redistribute_once(dwbc_batch *b, unsigned flags, dwbc_plan::Plan *planned) {
    // (DWBC_SOLVE_INIT clear is accepted: the one QP is strictly convex and starts cold either way)
    dwbc_plan::Plan p = redist_plan(b, (flags & DWBC_SOLVE_HQP) != 0);
    if (!p.row) return fail(p.err);
    if (flags & DWBC_SOLVE_REDUCED) return fail("redistribution of a supplied torque: not built on the reduced dynamics path");
    if (b->su.n_contacts < 1) return fail("no contact constraint");
    if (!b->tau_in_set) return fail("no torque input: call dwbc_batch_set_torque_input (or bind DWBC_IN_TORQUE) first");
    const bool grav = (flags & DWBC_REDIST_ADD_GRAVITY) != 0;
    if (grav && !(p = lean_plan(b, DWBC_LEAN_GRAV)).row) return fail(p.err);
    HIP_OK(hipSetDevice(b->device));
    if (!upload_inputs(b)) return 0;
    if (!send_inputs(b, {fld::kTauIn})) return 0;
    for (const int f : {DWBC_REDIST_TAU, DWBC_REDIST_CF, DWBC_REDIST_WRENCH, DWBC_REDIST_STATUS})
        if (!ensure_field(b, f)) return 0;
    if (grav && !lean_ensure(b, DWBC_LEAN_GRAV)) return 0;
    if (planned) *planned = p;
    return grav ? launch_grav(b, p, true) : launch_redistribute(b, p);
}

int dwbc_batch_redistribute(dwbc_batch *b, unsigned flags) { return redistribute_once(b, flags, nullptr); }
int dwbc_batch_time_redistribute(dwbc_batch *b, unsigned flags, int steps, float *ms) {
    dwbc_plan::Plan p{};
    const bool grav = (flags & DWBC_REDIST_ADD_GRAVITY) != 0;
    return time_launches(b, steps, ms, [&] { return redistribute_once(b, flags, &p); }, [&] { return grav ? launch_grav(b, p, true) : launch_redistribute(b, p); });
}
const char *dwbc_batch_redistribute_kernel_name(const dwbc_batch *b) { return plan_name(redist_plan(b, true), fld::kLeanCount); }

int dwbc_batch_copy_kinematics(dwbc_batch *dst, const dwbc_batch *src) {
    // RobotData::CopyKinematicsData (reference src/dwbc.cpp:1711-1762): state, contacts (with their flags), task spaces (with
    // their f*), torque limit and control time go to the target object, which then runs its own Calc* sequence.  Everything
    // derived (A_, A_inv_, link_, G_, CMM_, B_) is recomputed by the fused kernel from the copied state.
    if (!dst || !src) return fail("NULL batch");
    if (dst == src) return 1;
    if (dst->B != src->B || dst->n != src->n || dst->su.nb != src->su.nb) return fail("CopyKinematicsData: batch size / model mismatch");
    HIP_OK(hipSetDevice(dst->device));
    wait_uploads(dst);  // the target's mirrors are rewritten below
    if (dst->su.n_contacts != src->su.n_contacts) drop_instance_params(dst);  // (never copied; the target's own goes with its stride)
    drop_task_space(dst);  // (the task levels come with the set-up)
    drop_task_qp(dst);
    // (the per-instance body tables are never copied either: the model is no kinematics data, and the target keeps its own)
    dst->su = src->su;
    Buf &dq = dst->buf[fld::kQ];
    const Buf &sq = src->buf[fld::kQ];
    const size_t q_bytes = dwbc_batch_field_bytes(src, DWBC_IN_Q);
    dq.h = sq.h;
    dq.dirty = true;
    if (sq.bound() || sq.h.size() != q_bytes) {  // the source reads a caller-owned device buffer: device-to-device copy
        if (dq.bound()) release(dq);
        if (!ensure(dq, q_bytes)) return 0;
        HIP_OK(hipMemcpy(dq.d, sq.d, q_bytes, hipMemcpyDeviceToDevice));
        dq.h.assign(q_bytes);
        HIP_OK(hipMemcpy(dq.h.data(), sq.d, q_bytes, hipMemcpyDeviceToHost));
        dq.dirty = false;
    }
    // f* and flags: the target's own buffers, (re)allocated by upload_inputs; what a bound source holds is read back from its device buffer
    for (const int f : {DWBC_IN_FSTAR, DWBC_IN_CONTACT}) {
        const int slot = fld::find(f)->idx;
        Buf &d = dst->buf[slot];
        const Buf &sb = src->buf[slot];
        const size_t bytes = dwbc_batch_field_bytes(src, f);
        release(d);
        d.h = sb.h; d.dirty = true;
        if (sb.bound() && bytes > 0) {
            d.h.assign(bytes);
            HIP_OK(hipMemcpy(d.h.data(), sb.d, bytes, hipMemcpyDeviceToHost));
        }
    }
    // the contact capacity travels with the flags (a three-contact source would otherwise hand the two-contact product kernels rows
    // with three flags raised: status 0 on every such instance); after the flags, so that lowering is checked against the copied ones
    if (dst->max_active != src->max_active && !dwbc_batch_set_max_active_contacts(dst, src->max_active)) return 0;
    for (const int slot : {fld::kQdot, fld::kCtime, fld::kTraj, fld::kCustom}) {  // (send() sizes the device buffer by the mirror)
        dst->buf[slot].h = src->buf[slot].h;
        dst->buf[slot].dirty = !src->buf[slot].h.empty();
    }
    return 1;
}

int dwbc_batch_sync(dwbc_batch *b) {
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    return 1;
}

// device -> page-locked staging (asynchronous on the batch's stream, PCIe rate) -> the caller's memory
static int read_back(dwbc_batch *b, const void *src, void *out, size_t nbytes) {
    if (b->h_stage.size() < nbytes) b->h_stage.assign(nbytes);
    HIP_OK(hipMemcpyAsync(b->h_stage.data(), src, nbytes, hipMemcpyDeviceToHost, b->stream));
    HIP_OK(hipStreamSynchronize(b->stream));
    memcpy(out, b->h_stage.data(), nbytes);
    return 1;
}

int dwbc_batch_get(dwbc_batch *b, int field, void *out, size_t bytes) {
    const fld::Row *r = fld::find(field);
    const size_t need = dwbc_batch_field_bytes(b, field);
    if (need == 0) return fail("unknown field");
    if (bytes < need) return fail("output buffer too small");
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    auto d2h = [&](const void *src, size_t nbytes) -> int { return read_back(b, src, out, nbytes); };
    if (r->where == fld::kInSlot) {
        const void *src = b->buf[r->idx].d;
        return src || !r->absent ? d2h(src, need) : fail(r->absent);
    }
    if (r->where == fld::kTauPart) {
        // one third of the bytes over PCIe: the part (or the sum, getTorqueCommand-style) is formed on the device
        const size_t cnt = need / sizeof(double);
        if (!b->d_total) HIP_OK(hipMalloc(&b->d_total, need));
        hipLaunchKernelGGL(dwbc_tau_select, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, b->stream, (const double *)b->dev<double>(fld::kTau), b->d_total, b->m, cnt, r->idx);
        HIP_OK(hipGetLastError());
        return d2h(b->d_total, need);
    }
    if (!b->d_dump || !b->dump_on) return fail("intermediates need dwbc_batch_enable_dump(b, 1) before the solve");
    const size_t row = need / b->B, off = r->off ? (size_t)(b->dl.*(r->off)) : 0;
    HIP_OK(hipMemcpy2D(out, row, b->d_dump + off, (size_t)b->dl.total * sizeof(double), row, b->B, hipMemcpyDeviceToHost));
    return 1;
}

// the plan of the last accepted launch; before any solve, the one a full-model solve of the batch as it stands would get
static dwbc_plan::Plan report_plan(const dwbc_batch *b) {
    return b->last.row ? b->last : dwbc_plan::plan(plan_request(b, false), b->tables, b->n_tables);
}

const char *dwbc_batch_kernel_name(const dwbc_batch *b) {
    static thread_local char name[160];  // as rocprofv3 prints the instantiation
    const dwbc_plan::Plan p = report_plan(b);
    if (!p.row) return "";
    dwbc_plan::format_name(*p.row, name, sizeof name);
    return name;
}

int dwbc_batch_launch_info(const dwbc_batch *b, int *threads, int *lds) {
    const dwbc_plan::Plan p = report_plan(b);
    if (threads) *threads = p.row ? p.threads : kNT;
    if (lds) *lds = p.row ? p.lds : 0;
    return 1;
}

// ---- UpdateKinematics on its own for a set of queried links: the lean kernel of dwbc_link_query.h
int dwbc_batch_set_link_query(dwbc_batch *b, int n, const int32_t *links, const double *points, int want_jacobians) {
    if (n < 0 || n > kMaxLinkQuery) return fail("link query: at most 16 entries");
    if (n > 0 && !links) return fail("link query: links is NULL");
    const int nb = b->su.nb;
    for (int i = 0; i < n; i++) {
        if (links[i] < 0 || links[i] > nb) return fail("link query: link " + std::to_string(links[i]) + " is outside [0, " + std::to_string(nb) + "] (the last is the COM link)");
        if (links[i] == nb && points && (points[3 * i] != 0.0 || points[3 * i + 1] != 0.0 || points[3 * i + 2] != 0.0))
            return fail("link query: the COM link takes no point");
    }
    if (n > 0) {
        const dwbc_plan::Plan p = lean_plan(b, DWBC_LEAN_LINK_QUERY);
        if (!p.row) return fail(p.err);
    }
    b->lq_n = n;  // (sizes the outputs of the request below)
    for (int i = 0; i < n; i++) {
        b->lq_link[i] = links[i];
        for (int a = 0; a < 3; a++) b->lq_point[i][a] = points ? points[3 * i + a] : 0.0;
    }
    unsigned mask = n > 0 ? fld::kLean[DWBC_LEAN_LINK_QUERY].all() : 0u;  // an empty query drops the request and its buffers
    if (!want_jacobians) mask &= ~(1u << DWBC_LQ_JAC);
    return lean_request(b, DWBC_LEAN_LINK_QUERY, mask);
}

int dwbc_batch_update_kinematics(dwbc_batch *b) {
    if (!b->lean[DWBC_LEAN_LINK_QUERY].mask) return fail(fld::kLean[DWBC_LEAN_LINK_QUERY].no_request);
    const dwbc_plan::Plan p = lean_plan(b, DWBC_LEAN_LINK_QUERY);
    if (!p.row) return fail(p.err);
    HIP_OK(hipSetDevice(b->device));
    if (!send_inputs(b, {fld::kQdot, fld::kQ})) return 0;
    BatchIO io = lean_io(b);  // the state and the model; no buffer of the cycle or of the redistribution is named
    io.qdot = b->dev<double>(fld::kQdot);
    LinkQueryIO lq{};
    lq.n = b->lq_n;
    lq.nb = b->su.nb;
    lq.maxdepth = b->su.maxdepth;
    lq.want_jac = (b->lean[DWBC_LEAN_LINK_QUERY].mask >> DWBC_LQ_JAC) & 1u;
    for (int i = 0; i < b->lq_n; i++) {
        lq.link[i] = b->lq_link[i];
        lq.has_com = lq.has_com || b->lq_link[i] == b->su.nb;
        for (int a = 0; a < 3; a++) lq.point[i][a] = b->lq_point[i][a];
    }
    lq.pos = b->dev<double>(fld::kLqPos);
    lq.rot = b->dev<double>(fld::kLqRot);
    lq.vel = b->dev<double>(fld::kLqVel);
    lq.jac = lq.want_jac ? b->dev<double>(fld::kLqJac) : nullptr;
    void *args[] = {(void *)&io, (void *)&lq};
    if (!launch_kernel(b, p, args)) return 0;
    b->lean[DWBC_LEAN_LINK_QUERY].ran = true;
    return 1;
}

size_t dwbc_batch_link_query_bytes(const dwbc_batch *b, int what) { return lean_bytes(b, DWBC_LEAN_LINK_QUERY, what); }
int dwbc_batch_get_link_query(dwbc_batch *b, int what, void *out, size_t bytes) { return lean_get(b, DWBC_LEAN_LINK_QUERY, what, out, bytes); }
int dwbc_batch_bind_link_query(dwbc_batch *b, int what, void *p) { return lean_bind(b, DWBC_LEAN_LINK_QUERY, what, p); }
const char *dwbc_batch_link_query_kernel_name(const dwbc_batch *b) { return plan_name(lean_plan(b, DWBC_LEAN_LINK_QUERY), DWBC_LEAN_LINK_QUERY); }

// ---- the dynamics half of UpdateKinematics on its own (A_, A_inv_, B_, G_, CMM_, com_pos): the lean kernel of dwbc_dynamics.h
static_assert(kDynA == 1u << DWBC_DYN_A && kDynAInv == 1u << DWBC_DYN_A_INV && kDynB == 1u << DWBC_DYN_B && kDynG == 1u << DWBC_DYN_G &&
                  kDynCmm == 1u << DWBC_DYN_CMM && kDynCom == 1u << DWBC_DYN_COM, "DynIO::mask is 1u << dwbc_dynamics_output");
static int launch_dynamics(dwbc_batch *b, const dwbc_plan::Plan &p) {
    BatchIO io = lean_io(b);  // the state and the model; no buffer of the cycle, the redistribution, the gravity compensation or the link query is named
    io.qdot = b->dev<double>(fld::kQdot);
    DynIO dio{};
    dio.mask = b->lean[DWBC_LEAN_DYNAMICS].mask & ~(1u << DWBC_DYN_STATUS);
    dio.A = b->dev<double>(fld::kDyA);
    dio.A_inv = b->dev<double>(fld::kDyAInv);
    dio.Bv = b->dev<double>(fld::kDyB);
    dio.G = b->dev<double>(fld::kDyG);
    dio.CMM = b->dev<double>(fld::kDyCmm);
    dio.com = b->dev<double>(fld::kDyCom);
    dio.status = b->dev<int>(fld::kDyStatus);
    void *args[] = {(void *)&b->su, (void *)&io, (void *)&dio};
    if (!launch_kernel(b, p, args)) return 0;
    b->lean[DWBC_LEAN_DYNAMICS].ran = true;
    return 1;
}

// uploads whatever is pending of the state, launches once; *planned (optional): the plan of the launch, for a caller that repeats it
static int dynamics_once(dwbc_batch *b, dwbc_plan::Plan *planned) {
    if (!b->lean[DWBC_LEAN_DYNAMICS].mask) return fail(fld::kLean[DWBC_LEAN_DYNAMICS].no_request);
    const dwbc_plan::Plan p = lean_plan(b, DWBC_LEAN_DYNAMICS);
    if (!p.row) return fail(p.err);
    HIP_OK(hipSetDevice(b->device));
    if (!send_inputs(b, {fld::kQdot, fld::kQ})) return 0;
    if (planned) *planned = p;
    return launch_dynamics(b, p);
}

int dwbc_batch_set_dynamics_outputs(dwbc_batch *b, unsigned mask) { return lean_set_outputs(b, DWBC_LEAN_DYNAMICS, mask); }
int dwbc_batch_update_dynamics(dwbc_batch *b) { return dynamics_once(b, nullptr); }
int dwbc_batch_time_dynamics(dwbc_batch *b, int steps, float *ms) {
    dwbc_plan::Plan p{};
    return time_launches(b, steps, ms, [&] { return dynamics_once(b, &p); }, [&] { return launch_dynamics(b, p); });
}
size_t dwbc_batch_dynamics_bytes(const dwbc_batch *b, int what) { return lean_bytes(b, DWBC_LEAN_DYNAMICS, what); }
int dwbc_batch_get_dynamics(dwbc_batch *b, int what, void *out, size_t bytes) { return lean_get(b, DWBC_LEAN_DYNAMICS, what, out, bytes); }
int dwbc_batch_bind_dynamics(dwbc_batch *b, int what, void *p) { return lean_bind(b, DWBC_LEAN_DYNAMICS, what, p); }
const char *dwbc_batch_dynamics_kernel_name(const dwbc_batch *b) { return plan_name(lean_plan(b, DWBC_LEAN_DYNAMICS), DWBC_LEAN_DYNAMICS); }

// ---- SetContact + CalcContactConstraint on their own (J_C, Lambda_contact, J_C_INV_T, N_C, A_inv_N_C, W, W_inv, NwJw, contact frames):
// the lean kernel of dwbc_contact_space.h
static_assert(kCsJC == 1u << DWBC_CS_J_C && kCsLambda == 1u << DWBC_CS_LAMBDA_C && kCsJCInvT == 1u << DWBC_CS_J_C_INV_T && kCsNC == 1u << DWBC_CS_N_C &&
                  kCsAInvNC == 1u << DWBC_CS_A_INV_N_C && kCsW == 1u << DWBC_CS_W && kCsWInv == 1u << DWBC_CS_W_INV && kCsNwJw == 1u << DWBC_CS_NWJW &&
                  kCsPos == 1u << DWBC_CS_CONTACT_POS && kCsRot == 1u << DWBC_CS_CONTACT_ROT, "CsIO::mask is 1u << dwbc_contact_space_output");
static int launch_contact_space(dwbc_batch *b, const dwbc_plan::Plan &p) {
    BatchIO io = lean_io(b);  // the state, the flags and the model; no buffer of the cycle or of the other lean launches is named
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.hqp = 1;
    CsIO cio{};
    cio.mask = b->lean[DWBC_LEAN_CONTACT_SPACE].mask & ~(1u << DWBC_CS_STATUS);
    cio.J_C = b->dev<double>(fld::kCoJC);
    cio.Lambda_c = b->dev<double>(fld::kCoLambda);
    cio.J_C_INV_T = b->dev<double>(fld::kCoJCInvT);
    cio.N_C = b->dev<double>(fld::kCoNC);
    cio.A_inv_N_C = b->dev<double>(fld::kCoAInvNC);
    cio.W = b->dev<double>(fld::kCoW);
    cio.W_inv = b->dev<double>(fld::kCoWInv);
    cio.NwJw = b->dev<double>(fld::kCoNwJw);
    cio.pos = b->dev<double>(fld::kCoPos);
    cio.rot = b->dev<double>(fld::kCoRot);
    cio.status = b->dev<int>(fld::kCoStatus);
    void *args[] = {(void *)&b->su, (void *)&io, (void *)&cio};
    if (!launch_kernel(b, p, args)) return 0;
    b->lean[DWBC_LEAN_CONTACT_SPACE].ran = true;
    return 1;
}

// uploads whatever is pending of the state and the flags, launches once; *planned (optional): the plan of the launch, for a caller that repeats it
// (the plan's refusals come before the missing request here and after it in dynamics_once: callers see the order, so each family keeps its own)
static int contact_space_once(dwbc_batch *b, dwbc_plan::Plan *planned) {
    const dwbc_plan::Plan p = lean_plan(b, DWBC_LEAN_CONTACT_SPACE);
    if (!p.row) return fail(p.err);
    if (!b->lean[DWBC_LEAN_CONTACT_SPACE].mask) return fail(fld::kLean[DWBC_LEAN_CONTACT_SPACE].no_request);
    HIP_OK(hipSetDevice(b->device));
    if (!send_inputs(b, {fld::kQ, fld::kFlags})) return 0;
    if (!b->buf[fld::kFlags].d) return fail("no contact flags: call dwbc_batch_set_contact (or bind DWBC_IN_CONTACT) first");
    if (planned) *planned = p;
    return launch_contact_space(b, p);
}

int dwbc_batch_set_contact_space_outputs(dwbc_batch *b, unsigned mask) { return lean_set_outputs(b, DWBC_LEAN_CONTACT_SPACE, mask); }
int dwbc_batch_calc_contact_constraint(dwbc_batch *b) { return contact_space_once(b, nullptr); }
int dwbc_batch_time_contact_space(dwbc_batch *b, int steps, float *ms) {
    dwbc_plan::Plan p{};
    return time_launches(b, steps, ms, [&] { return contact_space_once(b, &p); }, [&] { return launch_contact_space(b, p); });
}
size_t dwbc_batch_contact_space_bytes(const dwbc_batch *b, int what) { return lean_bytes(b, DWBC_LEAN_CONTACT_SPACE, what); }
int dwbc_batch_get_contact_space(dwbc_batch *b, int what, void *out, size_t bytes) { return lean_get(b, DWBC_LEAN_CONTACT_SPACE, what, out, bytes); }
int dwbc_batch_bind_contact_space(dwbc_batch *b, int what, void *p) { return lean_bind(b, DWBC_LEAN_CONTACT_SPACE, what, p); }
const char *dwbc_batch_contact_space_kernel_name(const dwbc_batch *b) { return plan_name(lean_plan(b, DWBC_LEAN_CONTACT_SPACE), DWBC_LEAN_CONTACT_SPACE); }

// ---- SetTaskSpace + CalcTaskSpace on their own (J_task, Lambda_task, J_kt, Null_task per level): the lean kernel of dwbc_task_space.h.
// Its outputs are no family of kLean (they exist once per level, in the shape of the level's task dof): the table is dwbc_fields::kTaskSpace,
// the request and the "ran" flag dwbc_batch::ts, and what follows is the families' plumbing with a level beside the output
static_assert(kTsJTask == 1u << DWBC_TS_J_TASK && kTsLambda == 1u << DWBC_TS_LAMBDA_TASK && kTsJkt == 1u << DWBC_TS_J_KT && kTsNull == 1u << DWBC_TS_NULL_TASK,
              "TsIO::mask is 1u << dwbc_task_space_output");
static dwbc_plan::Plan task_space_plan(const dwbc_batch *b) {
    dwbc_plan::Request q = plan_request(b, false);
    q.task_space = true;
    return dwbc_plan::plan(q, b->tables, b->n_tables);
}
static int ts_slot(int level, int what) { return what == DWBC_TS_STATUS ? (int)fld::kTsStatusSlot : fld::kTaskSpaceRows[what].slot + level; }
// levels an output exists on: every one; Null_task all but the last; the status once
static int ts_levels(const dwbc_batch *b, int what) { return what == DWBC_TS_STATUS ? 1 : b->su.n_levels - (what == DWBC_TS_NULL_TASK ? 1 : 0); }

int dwbc_task_space_output_describe(int index, int n, int t, dwbc_field_info *out) {
    if (index < 0 || index >= fld::kTaskSpace.count || !out) return 0;
    const fld::LeanRow &r = fld::kTaskSpaceRows[index];
    *out = fld::describe(r.id, r.name, r.type, r.shape, dwbc_field_dims{n, 0, 0, 0}, 0, true, false, t);
    return 1;
}

size_t dwbc_batch_task_space_bytes(const dwbc_batch *b, int level, int what) {
    const fld::Family &f = fld::kTaskSpace;
    if (what < 0 || what >= f.count || !((b->ts.mask >> what) & 1u)) return 0;
    if (what == DWBC_TS_STATUS) level = 0;
    if (level < 0 || level >= ts_levels(b, what)) return 0;
    return (size_t)b->B * fld::elements(f.rows[what].shape, field_dims(b), 0, b->su.t_dof[level]) * fld::item_size(f.rows[what].type);
}

// why output `what` of `level` cannot be named (nullptr: it can)
static const char *ts_refusal(const dwbc_batch *b, int level, int what) {
    const fld::Family &f = fld::kTaskSpace;
    if (what < 0 || what >= f.count) return f.unknown;
    if (!b->ts.mask) return f.no_request;
    if (what != DWBC_TS_STATUS) {
        if (level < 0 || level >= b->su.n_levels) return "task space: no such task level";
        if (what == DWBC_TS_NULL_TASK && level == b->su.n_levels - 1) return "task space: the last level has no Null_task (the reference forms none: src/dwbc.cpp:804)";
    }
    if (!((b->ts.mask >> what) & 1u)) return f.not_asked;
    return nullptr;
}

int dwbc_batch_set_task_space_outputs(dwbc_batch *b, unsigned mask) {
    const fld::Family &f = fld::kTaskSpace;
    if (mask & ~f.all()) return fail(f.unknown_bit);
    if (mask) {
        const dwbc_plan::Plan p = task_space_plan(b);
        if (!p.row) return fail(p.err);
        mask |= 1u << f.status;
    }
    drop_task_space(b);  // (hipFree waits for the launches that write them)
    HIP_OK(hipSetDevice(b->device));
    b->ts.mask = mask;
    for (int w = 0; w < f.count; w++)
        for (int l = 0; l < ts_levels(b, w); l++)
            if (const size_t bytes = dwbc_batch_task_space_bytes(b, l, w))
                if (!ensure(b->buf[ts_slot(l, w)], bytes)) return 0;
    return 1;
}

int dwbc_batch_get_task_space(dwbc_batch *b, int level, int what, void *out, size_t bytes) {
    if (const char *why = ts_refusal(b, level, what)) return fail(why);
    if (!b->ts.ran) return fail(fld::kTaskSpace.not_run);
    const size_t need = dwbc_batch_task_space_bytes(b, level, what);
    if (bytes != need) return fail("task space: the host buffer has " + std::to_string(bytes) + " bytes, the output " + std::to_string(need));
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    return read_back(b, b->buf[ts_slot(level, what)].d, out, need);
}

int dwbc_batch_bind_task_space(dwbc_batch *b, int level, int what, void *p) {
    if (const char *why = ts_refusal(b, level, what)) return fail(why);
    HIP_OK(hipSetDevice(b->device));
    Buf &u = b->buf[ts_slot(level, what)];
    release(u);
    b->ts.ran = false;  // (what the batch's own buffer held is not in the new one)
    if (!p) return ensure(u, dwbc_batch_task_space_bytes(b, level, what));
    u.d = p;
    return 1;
}

static int launch_task_space(dwbc_batch *b, const dwbc_plan::Plan &p) {
    BatchIO io = lean_io(b);  // the state, the flags and the model; no buffer of the cycle or of the other lean launches is named
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.hqp = 1;
    TsIO tio{};
    tio.mask = b->ts.mask & ~(1u << DWBC_TS_STATUS);
    for (int l = 0; l < b->su.n_levels; l++) {
        tio.J_task[l] = b->dev<double>(ts_slot(l, DWBC_TS_J_TASK));
        tio.Lambda[l] = b->dev<double>(ts_slot(l, DWBC_TS_LAMBDA_TASK));
        tio.J_kt[l] = b->dev<double>(ts_slot(l, DWBC_TS_J_KT));
        tio.Null[l] = b->dev<double>(ts_slot(l, DWBC_TS_NULL_TASK));
    }
    tio.status = b->dev<int>(fld::kTsStatusSlot);
    tio.cs_mask = ts_contact_stage_mask(tio.mask);  // of the contact stage: the columns A^-1 N_c and, where a level reads it, W^+ (cs_out stays NULL)
    void *args[] = {(void *)&b->su, (void *)&io, (void *)&tio};
    if (!launch_kernel(b, p, args)) return 0;
    b->ts.ran = true;
    return 1;
}

// uploads whatever is pending of the state and the flags, launches once; *planned (optional): the plan of the launch, for a caller that repeats it
static int task_space_once(dwbc_batch *b, dwbc_plan::Plan *planned) {
    const dwbc_plan::Plan p = task_space_plan(b);
    if (!p.row) return fail(p.err);
    if (!b->ts.mask) return fail(fld::kTaskSpace.no_request);
    HIP_OK(hipSetDevice(b->device));
    if (!send_inputs(b, {fld::kQ, fld::kFlags})) return 0;
    if (b->su.n_contacts > 0 && !b->buf[fld::kFlags].d) return fail("no contact flags: call dwbc_batch_set_contact (or bind DWBC_IN_CONTACT) first");
    if (planned) *planned = p;
    return launch_task_space(b, p);
}

int dwbc_batch_calc_task_space(dwbc_batch *b) { return task_space_once(b, nullptr); }
int dwbc_batch_time_task_space(dwbc_batch *b, int steps, float *ms) {
    dwbc_plan::Plan p{};
    return time_launches(b, steps, ms, [&] { return task_space_once(b, &p); }, [&] { return launch_task_space(b, p); });
}
const char *dwbc_batch_task_space_kernel_name(const dwbc_batch *b) {
    static thread_local char name[160];
    const dwbc_plan::Plan p = task_space_plan(b);
    if (!p.row) { fail(p.err); return ""; }
    dwbc_plan::format_name(*p.row, name, sizeof name);
    return name;
}

// ---- CalcSingleTaskTorqueWithQP for one task level on its own: the lean kernel of dwbc_task_qp.h.  Its outputs are a table of their own
// (dwbc_fields::kTaskQp), the request, the level, the "ran" flag and which inputs exist dwbc_batch::tq; what follows is the task-space
// launch's plumbing with two inputs beside the outputs
static_assert(kTqFstarQp == 1u << DWBC_TQ_F_STAR_QP && kTqContactQp == 1u << DWBC_TQ_CONTACT_QP && kTqTorqueH == 1u << DWBC_TQ_TORQUE_H &&
                  kTqTorqueNullH == 1u << DWBC_TQ_TORQUE_NULL_H && kTqTorqueContact == 1u << DWBC_TQ_TORQUE_CONTACT, "TqIO::mask is 1u << dwbc_task_qp_output");
static dwbc_plan::Plan task_qp_plan(const dwbc_batch *b) {
    dwbc_plan::Request q = plan_request(b, false);
    q.task_qp = true;
    return dwbc_plan::plan(q, b->tables, b->n_tables);
}
// why the level cannot be solved by this launch (nullptr: it can)
static const char *tq_level_refusal(const dwbc_batch *b, int level) {
    if (level < 0 || level >= b->su.n_levels) return "single-level task QP: no such task level";
    for (int j = 0; j < b->su.t_nlinks[level]; j++)
        if (b->su.t_traj_slot[level][j] >= 0)
            return "single-level task QP: the level carries a trajectory (its f* is formed on the device by the cycle, not read from DWBC_IN_FSTAR)";
    return nullptr;
}
static size_t tq_input_bytes(const dwbc_batch *b, int which) {
    return (size_t)b->B * b->m * (which == DWBC_TQ_IN_NULL ? b->m : 1) * sizeof(double);
}

int dwbc_task_qp_output_describe(int index, int n, dwbc_field_info *out) {
    if (index < 0 || index >= fld::kTaskQp.count || !out) return 0;
    const fld::LeanRow &r = fld::kTaskQpRows[index];
    *out = fld::describe(r.id, r.name, r.type, r.shape, dwbc_field_dims{n, 0, 0, 0}, 0, true, false);
    return 1;
}

size_t dwbc_batch_task_qp_bytes(const dwbc_batch *b, int what) {
    const fld::Family &f = fld::kTaskQp;
    if (what < 0 || what >= f.count || !((b->tq.mask >> what) & 1u)) return 0;
    return (size_t)b->B * fld::elements(f.rows[what].shape, field_dims(b)) * fld::item_size(f.rows[what].type);
}

// why output `what` cannot be named (nullptr: it can)
static const char *tq_refusal(const dwbc_batch *b, int what) {
    const fld::Family &f = fld::kTaskQp;
    if (what < 0 || what >= f.count) return f.unknown;
    if (!b->tq.mask) return f.no_request;
    if (!((b->tq.mask >> what) & 1u)) return f.not_asked;
    return nullptr;
}

int dwbc_batch_set_task_qp(dwbc_batch *b, int level, unsigned mask) {
    const fld::Family &f = fld::kTaskQp;
    if (mask & ~f.all()) return fail(f.unknown_bit);
    if (mask) {
        const dwbc_plan::Plan p = task_qp_plan(b);
        if (!p.row) return fail(p.err);
        if (const char *why = tq_level_refusal(b, level)) return fail(why);
        mask |= 1u << f.status;
    }
    HIP_OK(hipSetDevice(b->device));
    for (int w = 0; w < f.count; w++) release(b->buf[f.rows[w].slot]);  // (hipFree waits for the launches that write them)
    b->tq.mask = mask;
    b->tq.level = mask ? level : 0;
    b->tq.ran = false;
    for (int w = 0; w < f.count; w++)
        if (const size_t bytes = dwbc_batch_task_qp_bytes(b, w))
            if (!ensure(b->buf[f.rows[w].slot], bytes)) {  // a failed allocation leaves no request behind: no launch may see a set bit without its buffer
                for (int v = 0; v < f.count; v++) release(b->buf[f.rows[v].slot]);
                b->tq.mask = 0;
                b->tq.level = 0;
                return 0;
            }
    return 1;
}

int dwbc_batch_set_task_qp_inputs(dwbc_batch *b, const double *torque_prev, const double *null) {
    if (!torque_prev) return fail("single-level task QP: torque_prev is NULL");
    Buf &up = b->buf[fld::kTqTorquePrev], &un = b->buf[fld::kTqNull];
    if (up.bound()) return fail("single-level task QP: torque_prev is bound to a device buffer");
    if (null && un.bound()) return fail("single-level task QP: the null matrix is bound to a device buffer");
    HIP_OK(hipSetDevice(b->device));
    wait_uploads(b);
    up.h.assign(torque_prev, tq_input_bytes(b, DWBC_TQ_IN_TORQUE_PREV));
    up.dirty = true;
    b->tq.prev_set = true;
    if (null) {
        un.h.assign(null, tq_input_bytes(b, DWBC_TQ_IN_NULL));
        un.dirty = true;
    } else {  // the identity: nothing is read
        release(un);  // (hipFree waits for the launches that read it)
        un.h.clear();
        un.dirty = false;
    }
    b->tq.null_set = null != nullptr;
    return 1;
}

int dwbc_batch_bind_task_qp_input(dwbc_batch *b, int which, void *p, size_t bytes) {
    if (which != DWBC_TQ_IN_TORQUE_PREV && which != DWBC_TQ_IN_NULL) return fail("single-level task QP: unknown input");
    const size_t need = tq_input_bytes(b, which);
    if (p && bytes != need) return fail("single-level task QP: the device buffer has " + std::to_string(bytes) + " bytes, the input " + std::to_string(need));
    HIP_OK(hipSetDevice(b->device));
    wait_uploads(b);
    Buf &u = b->buf[which == DWBC_TQ_IN_NULL ? fld::kTqNull : fld::kTqTorquePrev];
    release(u);
    u.h.clear();
    u.d = p;
    u.dirty = false;
    (which == DWBC_TQ_IN_NULL ? b->tq.null_set : b->tq.prev_set) = p != nullptr;
    return 1;
}

int dwbc_batch_get_task_qp(dwbc_batch *b, int what, void *out, size_t bytes) {
    if (const char *why = tq_refusal(b, what)) return fail(why);
    if (!b->tq.ran) return fail(fld::kTaskQp.not_run);
    const size_t need = dwbc_batch_task_qp_bytes(b, what);
    if (bytes != need) return fail("single-level task QP: the host buffer has " + std::to_string(bytes) + " bytes, the output " + std::to_string(need));
    HIP_OK(hipSetDevice(b->device));
    HIP_OK(hipStreamSynchronize(b->stream));
    return read_back(b, b->buf[fld::kTaskQpRows[what].slot].d, out, need);
}

int dwbc_batch_bind_task_qp(dwbc_batch *b, int what, void *p, size_t bytes) {
    if (const char *why = tq_refusal(b, what)) return fail(why);
    const size_t need = dwbc_batch_task_qp_bytes(b, what);
    if (p && bytes != need) return fail("single-level task QP: the device buffer has " + std::to_string(bytes) + " bytes, the output " + std::to_string(need));
    HIP_OK(hipSetDevice(b->device));
    Buf &u = b->buf[fld::kTaskQpRows[what].slot];
    release(u);
    b->tq.ran = false;  // (what the batch's own buffer held is not in the new one)
    if (!p) return ensure(u, need);
    u.d = p;
    return 1;
}

static int launch_task_qp(dwbc_batch *b, const dwbc_plan::Plan &p) {
    BatchIO io = lean_io(b);  // the state, the flags, f*, the per-instance parameters and the model; no output of the cycle or of the other lean launches is named
    io.flags = b->dev<unsigned char>(fld::kFlags);
    io.fstar = b->dev<double>(fld::kFstar);
    io.hqp = 1;
    io.inst_par = b->dev<double>(fld::kInstPar);
    Setup su_rec;
    TqIO qio{};
    qio.mask = b->tq.mask & ~(1u << DWBC_TQ_STATUS);
    qio.level = b->tq.level;
    qio.torque_prev = b->dev<double>(fld::kTqTorquePrev);
    qio.null = b->tq.null_set ? b->dev<double>(fld::kTqNull) : nullptr;
    qio.f_star_qp = b->dev<double>(fld::kTqFstarQp);
    qio.contact_qp = b->dev<double>(fld::kTqContactQp);
    qio.torque_h = b->dev<double>(fld::kTqTorqueH);
    qio.torque_null_h = b->dev<double>(fld::kTqTorqueNullH);
    qio.torque_contact = b->dev<double>(fld::kTqTorqueContact);
    qio.status = b->dev<int>(fld::kTqStatus);
    qio.cs_mask = kTqContactStageMask;  // of the contact stage: W^+ with what it needs, and NwJw (cs_out stays NULL)
    void *args[] = {(void *)launch_setup(b, io, su_rec), (void *)&io, (void *)&qio};
    if (!launch_kernel(b, p, args)) return 0;
    b->tq.ran = true;
    return 1;
}

// uploads whatever is pending of the state, the flags, f*, the per-instance parameters and the two inputs, launches once; *planned
// (optional): the plan of the launch, for a caller that repeats it
static int task_qp_once(dwbc_batch *b, dwbc_plan::Plan *planned) {
    const dwbc_plan::Plan p = task_qp_plan(b);
    if (!p.row) return fail(p.err);
    if (!b->tq.mask) return fail(fld::kTaskQp.no_request);
    if (const char *why = tq_level_refusal(b, b->tq.level)) return fail(why);  // (a trajectory may have been set on the level since the request)
    if (!b->tq.prev_set) return fail("single-level task QP: no torque_prev (call dwbc_batch_set_task_qp_inputs or bind DWBC_TQ_IN_TORQUE_PREV first)");
    HIP_OK(hipSetDevice(b->device));
    if (!send_inputs(b, {fld::kInstPar, fld::kQ, fld::kFlags, fld::kFstar, fld::kTqTorquePrev, fld::kTqNull})) return 0;
    if (b->su.n_contacts > 0 && !b->buf[fld::kFlags].d) return fail("no contact flags: call dwbc_batch_set_contact (or bind DWBC_IN_CONTACT) first");
    if (!b->buf[fld::kFstar].d) return fail("no f*: call dwbc_batch_set_fstar (or bind DWBC_IN_FSTAR) first");
    if (planned) *planned = p;
    return launch_task_qp(b, p);
}

int dwbc_batch_calc_single_task_torque_qp(dwbc_batch *b) { return task_qp_once(b, nullptr); }
int dwbc_batch_time_task_qp(dwbc_batch *b, int steps, float *ms) {
    dwbc_plan::Plan p{};
    return time_launches(b, steps, ms, [&] { return task_qp_once(b, &p); }, [&] { return launch_task_qp(b, p); });
}
const char *dwbc_batch_task_qp_kernel_name(const dwbc_batch *b) {
    static thread_local char name[160];
    const dwbc_plan::Plan p = task_qp_plan(b);
    if (!p.row) { fail(p.err); return ""; }
    dwbc_plan::format_name(*p.row, name, sizeof name);
    return name;
}

}  // extern "C"
