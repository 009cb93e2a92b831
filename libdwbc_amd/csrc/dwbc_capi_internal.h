// dwbc_capi_internal.h -- the opaque handles of include/dwbc_batch.h as the translation units of libdwbc_hip.so see them
// (dwbc_capi.hip: cycle kernels + batch API; dwbc_hqp_capi.hip: hierarchical-QP class + LQP configurator).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/dwbc_batch.h"
#include "dwbc_fields.h"
#include "dwbc_launch_plan.h"
#include "dwbc_model.h"
#include "dwbc_types.h"

namespace dwbc {
// host memory of a batch: the mirrors of the per-cycle inputs and the read-back staging are page-locked, so that hipMemcpyAsync on the
// batch's stream really is asynchronous and runs at PCIe rate (pageable memory goes through the runtime's own staging, synchronously:
// that is what the rarely written task-reference inputs keep, and why nothing waits for their upload before they are rewritten)
struct HostBytes {
    bool pinned = true;  // set before the first allocation only
    HostBytes() = default;
    HostBytes(const HostBytes &) = delete;
    HostBytes &operator=(const HostBytes &o) { return this != &o ? assign(o.p_, o.n_) : *this; }  // the contents; page-locked or not stays as it is here
    ~HostBytes() { clear(); }
    HostBytes &assign(const void *src, size_t n) {  // n bytes, a copy of src or (nullptr) zeros; the memory is kept while the size is
        if (n != n_) {
            if (p_) pinned ? (void)hipHostFree(p_) : free(p_);
            p_ = nullptr;
            n_ = 0;
            if (n && pinned && hipHostMalloc((void **)&p_, n, hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
            if (n && !pinned && !(p_ = (unsigned char *)malloc(n))) throw std::bad_alloc();
            n_ = n;
        }
        if (n) src ? (void)memcpy(p_, src, n) : (void)memset(p_, 0, n);
        return *this;
    }
    void assign(size_t n) { assign(nullptr, n); }
    void clear() { assign(nullptr, 0); }
    bool empty() const { return n_ == 0; }
    size_t size() const { return n_; }
    unsigned char *data() const { return p_; }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p_); }
    unsigned char operator[](size_t i) const { return p_[i]; }

private:
    unsigned char *p_ = nullptr;
    size_t n_ = 0;
};
// one device buffer of a batch (dwbc_fields::Slot): allocated by the batch or bound by the caller, with the host mirror it is uploaded
// from where it has one
struct Buf {
    void *d = nullptr;
    bool own = false;   // d was allocated by the batch (and is freed by it)
    size_t bytes = 0;   // size of that allocation
    HostBytes h;        // host mirror (empty: none, or not sized yet)
    bool dirty = false; // the mirror is newer than the device buffer
    bool bound() const { return d && !own; }
};
std::string &capi_err();  // thread-local last error (dwbc_last_error)
inline int capi_fail(const std::string &s) {
    capi_err() = s;
    return 0;
}
}  // namespace dwbc
#define HIP_OK(expr)                                                                                           \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return dwbc::capi_fail(std::string(#expr) + ": " + hipGetErrorString(e_));      \
    } while (0)

struct dwbc_model {
    dwbc::Model m;
};

struct dwbc_batch {
    const dwbc_model *model = nullptr;
    int B = 0, device = 0, n = 0, m = 0;
    dwbc::Setup su{};
    hipStream_t stream = nullptr;
    // the device buffers that are owned or bound, with their host mirrors (dwbc_capi.hip: ensure / release / send); indexed by slot
    dwbc::Buf buf[dwbc_fields::kSlotCount];
    template <class T>
    T *dev(int slot) const { return static_cast<T *>(buf[slot].d); }
    dwbc_batch() {
        for (int s : {dwbc_fields::kTraj, dwbc_fields::kCtime, dwbc_fields::kCustom}) buf[s].h.pinned = false;
        lean[DWBC_LEAN_GRAV].mask = dwbc_fields::kLean[DWBC_LEAN_GRAV].all();
    }
    double *d_dump = nullptr, *d_body = nullptr;
    int *d_topo = nullptr;
    bool dump_on = false;
    int dtype = 0;  // DWBC_F64 | DWBC_F32 (arithmetic type of the kernels; the boundary buffers are always double)
    float *f_body = nullptr;
    int max_active = 2;           // simultaneously active contacts per instance the batch solves (2: product kernels; 3: dwbc_cycle_gc.h)
    int hqp = 1;
    int warm = 0;           // last solve flags had DWBC_SOLVE_INIT clear
    bool ws_valid = false;  // diag holds the working sets of a full-build launch
    bool last_reduced = false;  // mode of the most recent dwbc_batch_solve (the LQP / JACC entry points need the matching cycle)
    // launch tables the planner chooses from, in its order of preference: built in (fp64, fp32, the task-space and the task-QP kernels of
    // translation units of their own, the per-instance-model build), then the loaded pack of the model's own tree, then the generic pack of
    // its size -- resolved once, at creation
    dwbc_plan::Table tables[7] = {};
    int n_tables = 0;
    bool tree_match = false;  // tables[] holds a pack compiled for this model's parent table
    dwbc_plan::Plan last{};   // plan of the last accepted launch (row == nullptr: none yet): kernel_name / launch_info report it
    std::vector<const void *> lds_attr_set;  // kernels whose dynamic-LDS attribute has been raised on this batch's device
    dwbc::HostBytes h_stage;  // read-back staging of dwbc_batch_get
    double *d_total = nullptr;                // B x m scratch of the DWBC_TAU_* getters
    double *d_jacc[dwbc::kMaxLevels] = {nullptr, nullptr, nullptr, nullptr};  // per task level: B x jacc_rec_size (dwbc_batch_solve_jacc)
    int *d_jacc_status = nullptr;             // kMaxLevels x B
    int jacc_n[dwbc::kMaxLevels] = {0, 0, 0, 0};  // system size each record was written with (n, or RS for dwbc_batch_solve_jacc_r)
    double *d_rrec = nullptr;                 // B x DumpLayout::make(RS).total: the reduced system in dump-record layout (dwbc_hqp.h)
    int rrec_n = 0;
    double *d_jacc_nc = nullptr;              // B x jacc_nc_rec_size (dwbc_batch_solve_jacc_r_nc)
    int *d_jacc_nc_status = nullptr;
    // the mirrors are page-locked, so an upload returns before the DMA engine has read them: this event is recorded behind the
    // host-to-device copies of a solve and waited for before anything rewrites a mirror (dwbc_batch_set_*, dwbc_batch_host_ptr)
    hipEvent_t ev_upload = nullptr;
    bool upload_pending = false;
    int n_cu = 0;  // compute units of the batch's device
    bool tau_in_set = false;  // dwbc_batch_redistribute has a torque input: set through the mirror (created with the batch) or bound
    // per lean launch (enum dwbc_lean_family): the request -- bit i set: output i of the family (dwbc_fields::kLean) is written, 0: none --
    // and whether a launch has filled the outputs.  Gravity compensation always writes all three; the link query pos | rot | vel, and jac
    // when it was set with Jacobians; the other two what dwbc_batch_set_*_outputs named, with the status
    struct {
        unsigned mask = 0;
        bool ran = false;
    } lean[dwbc_fields::kLeanCount];
    // the same for the task-space launch (dwbc_fields::kTaskSpace), whose outputs exist once per task level: what
    // dwbc_batch_set_task_space_outputs named, with the status; dropped when the task set-up changes
    struct {
        unsigned mask = 0;
        bool ran = false;
    } ts;
    // the same for the single-level task-QP launch (dwbc_fields::kTaskQp): the level and what dwbc_batch_set_task_qp named, with the status,
    // and which of its two inputs exist (set through a mirror or bound); dropped when the task set-up changes
    struct {
        unsigned mask = 0;
        int level = 0;
        bool ran = false;
        bool prev_set = false, null_set = false;
    } tq;
    // the entries of the link query (dwbc_batch_set_link_query)
    int lq_n = 0, lq_link[16] = {};
    double lq_point[16][3] = {};
    dwbc::DumpLayout dl{};
};

