// group_api.hip -- several GPUs behind the C ABI (BASELINE.json north_star: "the batch dimension shards
// trivially across 8 GPUs with an RCCL all-gather over xGMI only to collect per-instance optimal thrusts/costs for selection").
//
// ONE process, n devices: a brov_group owns one brov_solver per device (a contiguous shard of the batch, the first total % n
// shards one instance larger -- the partition of bluerov2_amd/distributed.py), one non-blocking stream per device and one RCCL
// communicator per device (ncclCommInitAll).  No communication during the solve.  brov_group_gather issues ONE ncclAllGather per
// device inside ncclGroupStart / ncclGroupEnd, on the devices' own streams, behind the solve:
//     BROV_GATHER_RECORDS   the 104-byte result records {u0, cost, kkt, status, qp_iter, thrusts} of every instance, to every device
//     BROV_GATHER_PACKED    one packed (cost, global index) pair per device (16 B): the local arg-min, for callers that need only
//                           the winner (SURVEY.md 8e's alternative)
// and brov_group_select_best finishes with the global arg-min of cost over the successful instances (BASELINE configs[3],
// "best-trajectory select").  This is the route for the reference's C++ callers (bluerov2_dob.cpp:270-451 runs in one process);
// bluerov2_amd/distributed.py (one process PER GPU on torch.distributed) stays as the second route.
//
// RCCL is resolved at run time (dlopen of librccl.so.1, the copy PyTorch may already have mapped): a process that never creates a
// group never loads it, and libbluerov2_nmpc.so has neither a link-time nor a build-time dependency on it (the few RCCL types this
// file needs are declared below, with the values of rccl.h 2.x).
//
// Second collective, BROV_COLLECTIVE_COPY (brov_group_create_ex / brov_group_create_rank_ex): the all-gather as device-to-device copies
// between the ranks' buffers -- every rank publishes its contribution behind an event on its own stream, every rank pulls the others'
// into its own `gathered` / `pairs` array on its own stream.  No RCCL involved, devices may repeat: W ranks on ONE GPU run exactly the
// bookkeeping of W GPUs (shard bounds by global rank, padded staging, rank-major gathered layout, packed pairs, select over W x slots,
// mailbox), which is how the 1-GPU test box executes this file with W > 1 (tests/test_gpu_group_loopback.py).  The ranks of a copy
// group must live in one process (they meet in a process-wide table keyed by the 128-byte id).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

// ---- what this file uses of rccl.h (resolved by dlsym; values as in RCCL 2.x) ----
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint8 = 1, ncclDouble = 8 } ncclDataType_t;

#include "../../include/bluerov2_nmpc.h"
#include "host_common.hpp"
#include "select_device.hpp"

using namespace brov;

static thread_local std::string g_gerr;
extern "C" const char* brov_group_last_error(void) { return g_gerr.c_str(); }

namespace {

struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    std::string why;
};

Rccl& rccl() {
    static Rccl r;
    if (r.handle || !r.why.empty()) return r;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        r.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (r.handle) break;
    }
    if (!r.handle) {
        const char* e = dlerror();   // once: the call clears the message
        r.why = std::string("librccl.so.1 could not be loaded: ") + (e ? e : "?");
        return r;
    }
#define SYM(field, name) r.field = (decltype(r.field))dlsym(r.handle, name); if (!r.field) { r.why = std::string("RCCL symbol missing: ") + name; r.handle = nullptr; return r; }
    SYM(CommInitAll, "ncclCommInitAll") SYM(CommInitRank, "ncclCommInitRank") SYM(GetUniqueId, "ncclGetUniqueId") SYM(CommDestroy, "ncclCommDestroy") SYM(AllGather, "ncclAllGather")
    SYM(GroupStart, "ncclGroupStart") SYM(GroupEnd, "ncclGroupEnd") SYM(GetVersion, "ncclGetVersion") SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    return r;
}

// ---- BROV_COLLECTIVE_COPY: where the ranks of one group meet (one table entry per 128-byte id; the brov_group objects that hold the
// ranks share it).  A rank publishes what it contributes (pointer + an event recorded on its stream behind the data) and counts the
// gathers it has entered / finished pulling; the other ranks wait for those counters on the host and for the events on their streams.
struct CopyPeer {
    bool present = false;
    int dev = -1;
    const brov_result* src_rec = nullptr;   // contribution to a BROV_GATHER_RECORDS gather: [Bmax] records (the solver's own array, or the padded staging copy)
    const double* src_pair = nullptr;       // ... to a BROV_GATHER_PACKED gather: (cost, global index)
    hipEvent_t ready = nullptr;             // recorded on the rank's stream behind its contribution
    hipEvent_t pulled = nullptr;            // ... behind its copies out of the other ranks' buffers
    long entered = 0, done = 0;             // gathers this rank has entered / has issued all pulls of
    int mode = -1;
};
struct CopyComm {
    std::mutex m;
    std::condition_variable cv;
    std::vector<CopyPeer> peer;             // by GLOBAL rank
    int joined = 0;
};
std::mutex g_copy_m;
std::map<std::string, std::shared_ptr<CopyComm>> g_copy;
std::atomic<int> kCopyWaitSeconds{60};       // a rank that does not show up within this time is reported, not waited for forever

// the calling thread's current device is the caller's business: every entry point that switches devices puts it back
struct DeviceKeeper {
    int d = -1;
    DeviceKeeper() { if (hipGetDevice(&d) != hipSuccess) { d = -1; (void)hipGetLastError(); } }
    ~DeviceKeeper() { if (d >= 0) (void)hipSetDevice(d); }
};

}  // namespace

constexpr int kSelBlocks = 64;   // blocks of group_select_kernel
struct GroupMail { brov_result rec; int32_t slot; int32_t seq; int32_t owner; int32_t pad; };   // what the select kernels deliver to the host (pinned), seq last

#define HIPCHK(call) BROV_HIPCHK(g_gerr, call)
#define GNCCL(call)                                                                         \
    do {                                                                                    \
        ncclResult_t r_ = (call);                                                           \
        if (r_ != ncclSuccess) { g_gerr = std::string(#call) + ": " + rccl().GetErrorString(r_); return BROV_ERR_HIP; } \
    } while (0)

static int pinned_mail(GroupMail** m) {
    if (hipHostMalloc((void**)m, sizeof(GroupMail), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *m = nullptr; g_gerr = "brov_group_create: allocation of a pinned mailbox failed"; return BROV_ERR_ALLOC; }
    std::memset(*m, 0, sizeof(GroupMail));
    return BROV_OK;
}

// one rank of the group that lives in this process: a device, its shard of the batch and everything the gather and the select keep there
struct GroupRank {
    int dev = -1, rank = -1;              // device ordinal, GLOBAL rank
    int lo = 0, cnt = 0;                  // its shard: instances [lo, lo + cnt) of the batch
    brov_solver* sol = nullptr;
    hipStream_t st = nullptr;
    ncclComm_t comm = nullptr;
    brov_result* stage = nullptr;         // [Bmax] (uneven shards only): the shard's records + never-selectable padding
    brov_result* gathered = nullptr;      // [W * Bmax]
    double *pair = nullptr, *pairs = nullptr;   // [2] local (cost, global index) and [W * 2] gathered
    int* best = nullptr;                  // [2]: arg-min scratch (winning slot, ticket of the select kernel)
    GroupMail* pmail = nullptr;           // pinned: the local winner's record, written by the pack kernel
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // solve start / end = gather start / gather end / select end
    // local rank 0, where the select runs: partial results of the select kernel's blocks, the winning record, the pinned mailbox they deliver into
    double* sel_cost = nullptr; int* sel_idx = nullptr; brov_result* sel_rec = nullptr;
    GroupMail* mail = nullptr;
    DeviceAllocs mem;

    const brov_result* contribution(bool even) const { return even ? brov_results_device(sol) : stage; }   // what a BROV_GATHER_RECORDS gather takes from this rank: [Bmax] records

    int create(int W, int Bmax, bool even, bool first, const brov_opts* opts) {
        if (hipSetDevice(dev) != hipSuccess) { (void)hipGetLastError(); g_gerr = "brov_group_create: hipSetDevice failed"; return BROV_ERR_HIP; }
        if (int rc = brov_create(&sol, dev, cnt, opts)) { g_gerr = std::string("brov_group_create: shard ") + std::to_string(rank) + ": " + brov_last_error(); return rc; }
        HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        if (int rc = mem.alloc(&gathered, (size_t)W * Bmax, g_gerr)) return rc;
        if (int rc = mem.alloc(&pair, 2 + 2 * (size_t)W, g_gerr)) return rc;
        pairs = pair + 2;
        if (int rc = mem.alloc(&best, 2, g_gerr)) return rc;
        HIPCHK(hipMemset(best, 0, 2 * sizeof(int)));
        if (int rc = pinned_mail(&pmail)) return rc;
        if (first) {
            if (int rc = mem.alloc(&sel_cost, kSelBlocks, g_gerr)) return rc;
            if (int rc = mem.alloc(&sel_idx, kSelBlocks, g_gerr)) return rc;
            if (int rc = mem.alloc(&sel_rec, 1, g_gerr)) return rc;
            if (int rc = pinned_mail(&mail)) return rc;
        }
        if (!even) {
            if (int rc = mem.alloc(&stage, (size_t)Bmax, g_gerr)) return rc;
            // padding records: status -1, cost NaN -- never selectable; only the first cnt slots are ever rewritten
            HIPCHK(hipMemset(stage, 0xFF, (size_t)Bmax * sizeof(brov_result)));
        }
        for (hipEvent_t& e : ev) HIPCHK(hipEventCreate(&e));
        return BROV_OK;
    }
    // safe on a rank that was built in part, or not at all
    void destroy() {
        if (dev >= 0) (void)hipSetDevice(dev);
        if (comm && rccl().handle) rccl().CommDestroy(comm);
        brov_destroy(sol);
        mem.free_all();
        if (pmail) (void)hipHostFree(pmail);
        if (mail) (void)hipHostFree(mail);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};

struct brov_group {
    // n = ranks of THIS process, one per local device; W = ranks of the whole group (= n for the one-process form; one process per GPU: n = 1,
    // W = world), r0 = global rank of local rank 0.  lo / cnt are indexed by GLOBAL rank; a local rank carries its own pair.
    int n = 0, W = 0, r0 = 0, total = 0, Bmax = 0;
    bool even = true;                     // all shards equally large: the records are gathered straight from the solvers' own arrays
    std::vector<int> lo, cnt;
    std::vector<GroupRank> ranks;         // the select runs on ranks[0]
    int32_t mail_seq = 0;
    int last_mode = -1;
    int collective = BROV_COLLECTIVE_RCCL;
    std::shared_ptr<CopyComm> cc;         // BROV_COLLECTIVE_COPY: the meeting point of the group's ranks
    std::string cc_key;
    long round = 0;                       // gathers entered by this process's ranks
    bool timing = true;
    bool ev_sel = false;                  // the select-end event of the current step has been recorded
    bool ev_solve = false, ev_gather = false;   // ... the solve's pair, the gather's end
};

// arg-min of cost over the eligible records (select_device.hpp: status SUCCESS and a finite cost) of a (padded) record array: slot ->
// (rank = slot / Bmax, i = slot % Bmax), valid while i < cnt[rank]; ties go to the lowest slot = lowest global index.  Up to kSelBlocks blocks
// scan the array (65 536 records of 104 B at BASELINE configs[3]: one block needs ~0.1 ms for them), the block that draws the last ticket
// reduces the partial results, and -- so that the host needs no copy command and no second round trip for the winner -- writes the winning
// slot AND its record into a pinned host mailbox, the sequence word last.  out[0] = winning slot or -1, best_dev = the record on the device.
__global__ __launch_bounds__(256) void group_select_kernel(const brov_result* __restrict__ rec, int slots, int* __restrict__ out, double* pc, int* pi,
                                                             unsigned* ticket, brov_result* best_dev, GroupMail* mail, int seq) {
    __shared__ bool last;
    double best = 0.0;
    int bi = -1;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < slots; k += gridDim.x * blockDim.x)   // ascending within a thread
        if (result_eligible(rec[k].status, rec[k].cost)) argmin_next(best, bi, rec[k].cost, k);
    block_argmin<256>(best, bi);
    if (threadIdx.x == 0) {
        pc[blockIdx.x] = best; pi[blockIdx.x] = bi;
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    bi = -1;
    if (threadIdx.x < gridDim.x) { best = ((volatile double*)pc)[threadIdx.x]; bi = ((volatile int*)pi)[threadIdx.x]; }
    block_argmin<256>(best, bi);
    const int slot = bi;
    if (slot >= 0 && threadIdx.x < kResultWords) {
        const unsigned long long v = result_word(rec + slot, threadIdx.x);
        result_word(best_dev, threadIdx.x) = v;
        if (mail) result_word(&mail->rec, threadIdx.x) = v;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = slot;
        *ticket = 0;   // the next launch on this stream
        if (mail) {
            mail->slot = slot;
            __threadfence_system();
            *(volatile int32_t*)&mail->seq = seq;
        }
    }
}
// the local arg-min as a packed pair: pair[0] = cost (+inf when no record qualifies), pair[1] = global index (exact in a double).  The
// winner's whole record goes into the device's own pinned mailbox on the way (system-scope fence ahead of the pair: whoever learns the
// pair through the all-gather finds the record in place).
__global__ __launch_bounds__(256) void group_pack_kernel(const brov_result* __restrict__ rec, int n, int lo, double* __restrict__ pair, GroupMail* mail) {
    double best = 0.0;
    int w = -1;
    for (int k = threadIdx.x; k < n; k += blockDim.x)   // ascending within a thread
        if (result_eligible(rec[k].status, rec[k].cost)) argmin_next(best, w, rec[k].cost, k);
    block_argmin<256>(best, w);
    if (w >= 0 && threadIdx.x < kResultWords) result_word(&mail->rec, threadIdx.x) = result_word(rec + w, threadIdx.x);
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        mail->slot = w >= 0 ? lo + w : -1;
        __threadfence_system();
        pair[0] = w >= 0 ? best : __builtin_inf();
        pair[1] = w >= 0 ? (double)(lo + w) : -1.0;
    }
}
// the gathered pairs -> owner rank, global index and cost of the global winner, into the host mailbox (one wave; shards hold ascending
// index ranges, so the first minimal cost in rank order is the lowest index).  A pair is no record: its +inf cost with index -1 says "no
// winner on that rank", and every other pair carries the finite cost of an eligible record.
__global__ void group_pairs_kernel(const double* __restrict__ pairs, int W, GroupMail* mail, int seq) {
    if (threadIdx.x != 0) return;
    int owner = -1;
    for (int r = 0; r < W; r++)
        if (pairs[2 * r + 1] >= 0.0 && (owner < 0 || pairs[2 * r] < pairs[2 * owner])) owner = r;
    mail->owner = owner;
    mail->slot = owner >= 0 ? (int)pairs[2 * owner + 1] : -1;
    mail->rec.cost = owner >= 0 ? pairs[2 * owner] : 0.0;
    __threadfence_system();
    *(volatile int32_t*)&mail->seq = seq;
}

// poll the sequence word of rank 0's mailbox; the stream is queried now and then, so that a launch that ended without delivering (a
// device fault) turns into an error instead of a hang
static int mail_wait(GroupRank& r0, int32_t seq) {
    volatile int32_t* pf = (volatile int32_t*)&r0.mail->seq;
    for (unsigned long spin = 1; *pf != seq; spin++) {
        if ((spin & 0x3ff) == 0) {
            const hipError_t q = hipStreamQuery(r0.st);
            if (q == hipSuccess) {   // the launch is over: everything it wrote is visible
                if (*pf != seq) { g_gerr = "brov_group_select_best: the select kernel ended without delivering"; return BROV_ERR_HIP; }
            } else if (q != hipErrorNotReady) {
                g_gerr = std::string("brov_group_select_best: ") + hipGetErrorString(q);
                (void)hipGetLastError();
                return BROV_ERR_HIP;
            }
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return BROV_OK;
}

// one delivery through rank 0's pinned mailbox: the next sequence number, `launch(rank 0, number)` enqueues the kernel that writes the mailbox
// and the number last, the select-end event, and the host polls the sequence word: no copy command, no stream synchronisation on the way back
template <class Launch>
static int deliver(brov_group* g, Launch launch) {
    GroupRank& r0 = g->ranks[0];
    HIPCHK(hipSetDevice(r0.dev));
    g->mail_seq = g->mail_seq == 0x7fffffff ? 1 : g->mail_seq + 1;
    launch(r0, g->mail_seq);
    HIPCHK(hipGetLastError());
    if (g->timing) { HIPCHK(hipEventRecord(r0.ev[3], r0.st)); g->ev_sel = true; }
    return mail_wait(r0, g->mail_seq);
}

extern "C" {

int brov_group_rccl_version(int* version) {
    Rccl& r = rccl();
    if (!r.handle) { g_gerr = r.why; return BROV_ERR_HIP; }
    int v = 0;
    if (r.GetVersion(&v) != ncclSuccess) { g_gerr = "ncclGetVersion failed"; return BROV_ERR_HIP; }
    if (version) *version = v;
    return BROV_OK;
}

void brov_group_destroy(brov_group* g) {
    if (!g) return;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks) {   // everything this process's ranks have enqueued is over before anything is taken apart
        if (r.dev >= 0) hipSetDevice(r.dev);
        if (r.st) hipStreamSynchronize(r.st);
    }
    if (g->cc) {   // leave the copy collective's table (the other ranks must have finished the gathers they share with this one)
        {
            std::lock_guard<std::mutex> lk(g->cc->m);
            for (GroupRank& r : g->ranks) {
                if (r.rank >= (int)g->cc->peer.size() || !g->cc->peer[r.rank].present || g->cc->peer[r.rank].src_pair != r.pair) continue;   // not this rank's entry
                CopyPeer& me = g->cc->peer[r.rank];
                if (me.ready) hipEventDestroy(me.ready);
                if (me.pulled) hipEventDestroy(me.pulled);
                me = CopyPeer();
                g->cc->joined--;
            }
        }
        std::lock_guard<std::mutex> lk(g_copy_m);
        auto it = g_copy.find(g->cc_key);
        if (it != g_copy.end() && it->second == g->cc && g->cc->joined <= 0) g_copy.erase(it);
        g->cc.reset();
    }
    for (GroupRank& r : g->ranks) r.destroy();
    delete g;
}

// common part of the two creators: local devices dev[0..n), global ranks r0 .. r0 + n - 1 of W, instances per global rank in cnt[W]
static int group_build(brov_group** out, const int* devices, int n, int W, int r0, const std::vector<int>& cnt, const brov_opts* opts,
                       const ncclUniqueId* id, int collective) {
    if (collective != BROV_COLLECTIVE_RCCL && collective != BROV_COLLECTIVE_COPY) { g_gerr = "brov_group_create: unknown collective"; return BROV_ERR_ARG; }
    const bool copy = collective == BROV_COLLECTIVE_COPY;
    DeviceKeeper keep;
    for (int d = 0; d < n; d++) {
        if (!brov::usable_device(devices[d])) {
            g_gerr = "brov_group_create: no usable HIP device at ordinal " + std::to_string(devices[d]) + " (this library has no CPU fallback)";
            return BROV_ERR_NO_DEVICE;
        }
        for (int e = 0; e < d && !copy; e++)
            if (devices[e] == devices[d]) { g_gerr = "brov_group_create: a device may appear once (one RCCL rank per GPU; BROV_COLLECTIVE_COPY lifts this)"; return BROV_ERR_ARG; }
    }
    Rccl* Rp = copy ? nullptr : &rccl();
    if (Rp && !Rp->handle) { g_gerr = "brov_group_create: " + Rp->why; return BROV_ERR_HIP; }
    brov_group* g = new brov_group();
    g->n = n; g->W = W; g->r0 = r0; g->collective = collective;
    g->cnt = cnt; g->lo.assign(W, 0);
    for (int r = 0; r < W; r++) {
        g->lo[r] = r ? g->lo[r - 1] + g->cnt[r - 1] : 0;
        if (g->cnt[r] > g->Bmax) g->Bmax = g->cnt[r];
        g->even = g->even && g->cnt[r] == g->cnt[0];
    }
    g->total = g->lo[W - 1] + g->cnt[W - 1];
    g->ranks.resize(n);
    auto fail = [&](int rc) { brov_group_destroy(g); return rc; };
    for (int d = 0; d < n; d++) {
        GroupRank& r = g->ranks[d];
        r.dev = devices[d]; r.rank = r0 + d; r.lo = g->lo[r.rank]; r.cnt = g->cnt[r.rank];
        if (int rc = r.create(W, g->Bmax, g->even, d == 0, opts)) return fail(rc);
    }
    if (copy) {   // join the table entry of this group's id (the one-process form has an id of its own)
        g->cc_key = id ? std::string(id->internal, sizeof(id->internal)) : "one-process group " + std::to_string((unsigned long long)(uintptr_t)g);
        {
            std::lock_guard<std::mutex> lk(g_copy_m);
            std::shared_ptr<CopyComm>& sp = g_copy[g->cc_key];
            if (!sp) { sp = std::make_shared<CopyComm>(); sp->peer.resize(W); }
            g->cc = sp;
        }
        std::unique_lock<std::mutex> lk(g->cc->m);
        if ((int)g->cc->peer.size() != W) { lk.unlock(); g_gerr = "brov_group_create_rank: the ranks of this id disagree about the world size"; return fail(BROV_ERR_ARG); }
        for (GroupRank& r : g->ranks)
            if (g->cc->peer[r.rank].present) { lk.unlock(); g_gerr = "brov_group_create_rank: rank " + std::to_string(r.rank) + " of this id exists already"; return fail(BROV_ERR_ARG); }
        for (GroupRank& r : g->ranks) {
            CopyPeer& me = g->cc->peer[r.rank];
            me.dev = r.dev;
            me.src_rec = r.contribution(g->even);
            me.src_pair = r.pair;
            bool ok = hipSetDevice(r.dev) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&me.ready, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&me.pulled, hipEventDisableTiming) == hipSuccess;
            if (!ok) { lk.unlock(); g_gerr = "brov_group_create: events of the copy collective"; return fail(BROV_ERR_HIP); }
            me.present = true;
            g->cc->joined++;
        }
        g->cc->cv.notify_all();
    } else {
        Rccl& R = *Rp;
        ncclResult_t nr;
        if (id) {   // one process per GPU: this process is rank r0 of W
            if (hipSetDevice(g->ranks[0].dev) != hipSuccess) { g_gerr = "brov_group_create_rank: hipSetDevice failed"; return fail(BROV_ERR_HIP); }
            nr = R.CommInitRank(&g->ranks[0].comm, W, *id, r0);
        } else {
            std::vector<ncclComm_t> comm(n, nullptr);
            nr = R.CommInitAll(comm.data(), n, devices);
            for (int d = 0; d < n; d++) g->ranks[d].comm = comm[d];
        }
        if (nr != ncclSuccess) { g_gerr = std::string("brov_group_create: RCCL communicator set-up: ") + R.GetErrorString(nr); return fail(BROV_ERR_HIP); }
    }
    *out = g;
    return BROV_OK;
}

int brov_group_create_ex(brov_group** out, const int* devices, int n, int total, const brov_opts* opts, int collective) {
    if (!out || !devices || !opts || n < 1 || n > 64 || total < n) { g_gerr = "brov_group_create: bad argument (1 <= n <= 64 devices, at least one instance each)"; return BROV_ERR_ARG; }
    std::vector<int> cnt(n);
    for (int d = 0; d < n; d++) cnt[d] = total / n + (d < total % n ? 1 : 0);
    return group_build(out, devices, n, n, 0, cnt, opts, nullptr, collective);
}
int brov_group_create(brov_group** out, const int* devices, int n, int total, const brov_opts* opts) {
    return brov_group_create_ex(out, devices, n, total, opts, BROV_COLLECTIVE_RCCL);
}

// ---- one process per GPU: the same group, each process holding ONE rank of it ----------------------------------------------------
int brov_group_unique_id(char id[128]) {
    Rccl& R = rccl();
    if (!R.handle) { g_gerr = R.why; return BROV_ERR_HIP; }
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    ncclUniqueId u;
    if (!id || R.GetUniqueId(&u) != ncclSuccess) { g_gerr = "ncclGetUniqueId failed"; return BROV_ERR_HIP; }
    std::memcpy(id, &u, 128);
    return BROV_OK;
}
int brov_group_create_rank_ex(brov_group** out, int device, int rank, int world, const char id[128], const int* counts, const brov_opts* opts, int collective) {
    if (!out || !id || !counts || !opts || world < 1 || rank < 0 || rank >= world) { g_gerr = "brov_group_create_rank: bad argument"; return BROV_ERR_ARG; }
    std::vector<int> cnt(counts, counts + world);
    for (int r = 0; r < world; r++)
        if (cnt[r] < 1) { g_gerr = "brov_group_create_rank: every rank needs at least one instance"; return BROV_ERR_ARG; }
    ncclUniqueId u;
    std::memcpy(&u, id, 128);
    return group_build(out, &device, 1, world, rank, cnt, opts, &u, collective);
}
int brov_group_create_rank(brov_group** out, int device, int rank, int world, const char id[128], const int* counts, const brov_opts* opts) {
    return brov_group_create_rank_ex(out, device, rank, world, id, counts, opts, BROV_COLLECTIVE_RCCL);
}
int brov_group_collective(const brov_group* g) { return g ? g->collective : -1; }
int brov_group_set_copy_wait_seconds(int seconds) { if (seconds < 1) return BROV_ERR_ARG; kCopyWaitSeconds = seconds; return BROV_OK; }

int brov_group_size(const brov_group* g) { return g ? g->n : 0; }          /* devices of this process */
int brov_group_world(const brov_group* g) { return g ? g->W : 0; }         /* ranks of the whole group */
int brov_group_first_rank(const brov_group* g) { return g ? g->r0 : 0; }
int brov_group_total(const brov_group* g) { return g ? g->total : 0; }
brov_solver* brov_group_solver(brov_group* g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ranks[rank].sol : nullptr; }
void* brov_group_stream(brov_group* g, int rank) { return (g && rank >= 0 && rank < g->n) ? (void*)g->ranks[rank].st : nullptr; }
int brov_group_shard(const brov_group* g, int rank, int* lo, int* hi) {
    if (!g || rank < 0 || rank >= g->W) return BROV_ERR_ARG;   /* GLOBAL rank */
    if (lo) *lo = g->lo[rank];
    if (hi) *hi = g->lo[rank] + g->cnt[rank];
    return BROV_OK;
}

// ---- whole-batch setters: global HOST arrays, sliced per shard -------------------------------------------------------------
int brov_group_set_x0_host(brov_group* g, const double* x0) {
    if (!g || !x0) return BROV_ERR_ARG;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks)
        if (int rc = brov_set_x0_host(r.sol, x0 + (size_t)r.lo * 12)) { g_gerr = brov_last_error(); return rc; }
    return BROV_OK;
}
int brov_group_set_params_host(brov_group* g, const double* p, int per_stage) {
    if (!g || !p) return BROV_ERR_ARG;
    DeviceKeeper keep;
    const size_t row = per_stage ? (size_t)(brov_horizon(g->ranks[0].sol) + 1) * 16 : 16;
    for (GroupRank& r : g->ranks)
        if (int rc = brov_set_params_host(r.sol, p + (size_t)r.lo * row, per_stage)) { g_gerr = brov_last_error(); return rc; }
    return BROV_OK;
}
int brov_group_set_yref_host(brov_group* g, const double* yref, int shared) {
    if (!g || !yref) return BROV_ERR_ARG;
    DeviceKeeper keep;
    const size_t row = (size_t)(brov_horizon(g->ranks[0].sol) + 1) * 16;
    for (GroupRank& r : g->ranks)
        if (int rc = brov_set_yref_host(r.sol, shared ? yref : yref + (size_t)r.lo * row, shared)) { g_gerr = brov_last_error(); return rc; }
    return BROV_OK;
}
int brov_group_set_candidate_params_host(brov_group* g, int kind, const double* p0, const double* p1, const double* phase) {
    if (!g || !p0 || !p1 || !phase) return BROV_ERR_ARG;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks)
        if (int rc = brov_set_candidate_params_host(r.sol, kind, p0 + r.lo, p1 + r.lo, phase + r.lo)) { g_gerr = brov_last_error(); return rc; }
    return BROV_OK;
}
int brov_group_set_yref_candidates(brov_group* g, double t0, double dt) {   // one window kernel per device, on the device's stream
    if (!g) return BROV_ERR_ARG;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks)
        if (int rc = brov_set_yref_candidates(r.sol, t0, dt, r.st)) { g_gerr = brov_last_error(); return rc; }
    return BROV_OK;
}

int brov_group_enable_timing(brov_group* g, int on) { if (!g) return BROV_ERR_ARG; g->timing = on != 0; return BROV_OK; }

// BROV_COLLECTIVE_COPY, with c.m held: wait until every rank of the group is present and its counter `member` (entered / done) has reached
// `round`.  A rank that does not get there within the collective's time limit is named in the error, not waited for forever.
static int wait_for_ranks(CopyComm& c, std::unique_lock<std::mutex>& lk, long round, long CopyPeer::*member, const char* what) {
    int missing = -1;
    const bool ok = c.cv.wait_for(lk, std::chrono::seconds(kCopyWaitSeconds.load()), [&] {
        for (int r = 0; r < (int)c.peer.size(); r++)
            if (!c.peer[r].present || c.peer[r].*member < round) { missing = r; return false; }
        return true;
    });
    if (!ok) { g_gerr = "copy collective: rank " + std::to_string(missing) + what + std::to_string(round); return BROV_ERR_HIP; }
    return BROV_OK;
}

// BROV_COLLECTIVE_COPY: before a rank rewrites what it contributed to the last gather (its records: the next solve; its staging copy /
// its pair: the next gather), every rank has pulled it -- waited for on the host until the pulls are enqueued, on the streams until
// they have run.  (RCCL needs nothing of the kind: its all-gather ends on all streams together.)
static int copy_fence(brov_group* g) {
    if (!g->cc || g->round == 0) return BROV_OK;
    CopyComm& c = *g->cc;
    {
        std::unique_lock<std::mutex> lk(c.m);
        if (int rc = wait_for_ranks(c, lk, g->round, &CopyPeer::done, " has not finished gather ")) return rc;
    }
    for (GroupRank& me : g->ranks) {
        HIPCHK(hipSetDevice(me.dev));
        for (int r = 0; r < g->W; r++)
            if (r != me.rank) HIPCHK(hipStreamWaitEvent(me.st, c.peer[r].pulled, 0));
    }
    return BROV_OK;
}

// the all-gather as copies (see the head of the file): publish, meet, pull
static int copy_gather(brov_group* g, int mode) {
    CopyComm& c = *g->cc;
    const size_t rec = sizeof(brov_result);
    const long round = ++g->round;
    for (GroupRank& me : g->ranks) {
        HIPCHK(hipSetDevice(me.dev));
        HIPCHK(hipEventRecord(c.peer[me.rank].ready, me.st));
    }
    {
        std::unique_lock<std::mutex> lk(c.m);
        for (GroupRank& me : g->ranks) { c.peer[me.rank].entered = round; c.peer[me.rank].mode = mode; }
        c.cv.notify_all();
        // every rank has entered this gather: what a collective waits for on the device is waited for on the host here
        if (int rc = wait_for_ranks(c, lk, round, &CopyPeer::entered, " did not enter gather ")) return rc;
        for (int r = 0; r < g->W; r++)
            if (c.peer[r].entered == round && c.peer[r].mode != mode) { g_gerr = "copy collective: the ranks disagree about the gather mode"; return BROV_ERR_ARG; }
    }
    for (GroupRank& me : g->ranks) {
        HIPCHK(hipSetDevice(me.dev));
        for (int r = 0; r < g->W; r++) {
            if (r != me.rank) HIPCHK(hipStreamWaitEvent(me.st, c.peer[r].ready, 0));
            if (mode == BROV_GATHER_RECORDS)
                HIPCHK(hipMemcpyAsync(me.gathered + (size_t)r * g->Bmax, c.peer[r].src_rec, (size_t)g->Bmax * rec, hipMemcpyDefault, me.st));
            else
                HIPCHK(hipMemcpyAsync(me.pairs + 2 * r, c.peer[r].src_pair, 2 * sizeof(double), hipMemcpyDefault, me.st));
        }
        HIPCHK(hipEventRecord(c.peer[me.rank].pulled, me.st));
    }
    {
        std::lock_guard<std::mutex> lk(c.m);
        for (GroupRank& me : g->ranks) c.peer[me.rank].done = round;
        c.cv.notify_all();
    }
    return BROV_OK;
}

int brov_group_solve(brov_group* g) {
    if (!g) return BROV_ERR_ARG;
    DeviceKeeper keep;
    if (int rc = copy_fence(g)) return rc;
    for (GroupRank& r : g->ranks) {
        HIPCHK(hipSetDevice(r.dev));
        if (g->timing) HIPCHK(hipEventRecord(r.ev[0], r.st));
        if (int rc = brov_solve(r.sol, r.st)) { g_gerr = brov_last_error(); return rc; }
        if (g->timing) HIPCHK(hipEventRecord(r.ev[1], r.st));
    }
    g->last_mode = -1;
    g->ev_sel = false; g->ev_gather = false; g->ev_solve = g->timing;
    return BROV_OK;
}

int brov_group_gather(brov_group* g, int mode) {
    if (!g || (mode != BROV_GATHER_RECORDS && mode != BROV_GATHER_PACKED)) return BROV_ERR_ARG;
    DeviceKeeper keep;
    const size_t rec = sizeof(brov_result);
    if (int rc = copy_fence(g)) return rc;
    // what each rank contributes, produced on its own stream behind the solve
    for (GroupRank& r : g->ranks) {
        HIPCHK(hipSetDevice(r.dev));
        // (timing: the solve's end event doubles as the gather's start)
        if (mode == BROV_GATHER_RECORDS) {
            if (!g->even) HIPCHK(hipMemcpyAsync(r.stage, brov_results_device(r.sol), (size_t)r.cnt * rec, hipMemcpyDeviceToDevice, r.st));
        } else {
            hipLaunchKernelGGL(group_pack_kernel, dim3(1), dim3(256), 0, r.st, brov_results_device(r.sol), r.cnt, r.lo, r.pair, r.pmail);
            HIPCHK(hipGetLastError());
        }
    }
    if (g->cc) {
        if (int rc = copy_gather(g, mode)) return rc;
    } else {
        Rccl& R = rccl();
        GNCCL(R.GroupStart());
        for (GroupRank& r : g->ranks) {
            const ncclResult_t nr = mode == BROV_GATHER_RECORDS ? R.AllGather(r.contribution(g->even), r.gathered, (size_t)g->Bmax * rec, ncclUint8, r.comm, r.st)
                                                                : R.AllGather(r.pair, r.pairs, 2, ncclDouble, r.comm, r.st);
            if (nr != ncclSuccess) { R.GroupEnd(); g_gerr = std::string("ncclAllGather: ") + R.GetErrorString(nr); return BROV_ERR_HIP; }
        }
        GNCCL(R.GroupEnd());
    }
    if (g->timing)
        for (GroupRank& r : g->ranks) { HIPCHK(hipSetDevice(r.dev)); HIPCHK(hipEventRecord(r.ev[2], r.st)); }
    g->ev_gather = g->timing && g->ev_solve;
    g->last_mode = mode;
    return BROV_OK;
}

int brov_group_synchronize(brov_group* g) {
    if (!g) return BROV_ERR_ARG;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks) { HIPCHK(hipSetDevice(r.dev)); HIPCHK(hipStreamSynchronize(r.st)); }
    return BROV_OK;
}

static int slot_to_global(const brov_group* g, int slot) {
    if (slot < 0) return -1;
    const int r = slot / g->Bmax, i = slot % g->Bmax;
    return (r < g->W && i < g->cnt[r]) ? g->lo[r] + i : -1;
}

int brov_group_select_best(brov_group* g, int* best_index, brov_result* best) {
    if (!g || !best_index) return BROV_ERR_ARG;
    if (g->last_mode < 0) { g_gerr = "brov_group_select_best: call brov_group_gather first"; return BROV_ERR_ARG; }
    DeviceKeeper keep;
    *best_index = -1;
    const GroupMail* mail = g->ranks[0].mail;
    if (g->last_mode == BROV_GATHER_RECORDS) {
        // every rank holds all records: rank 0 selects (any would do; the others only finish their gather -- their streams order whatever is
        // enqueued next behind it).  The kernel delivers the winning slot and its record.
        const int slots = g->W * g->Bmax;
        int nb = (slots + 1023) / 1024;
        nb = nb < 1 ? 1 : (nb > kSelBlocks ? kSelBlocks : nb);
        if (int rc = deliver(g, [&](GroupRank& r, int32_t seq) {
                hipLaunchKernelGGL(group_select_kernel, dim3(nb), dim3(256), 0, r.st, r.gathered, slots, r.best, r.sel_cost, r.sel_idx, (unsigned*)(r.best + 1),
                                   r.sel_rec, r.mail, seq);
            })) return rc;
        *best_index = slot_to_global(g, mail->slot);
        if (best && mail->slot >= 0) std::memcpy(best, &mail->rec, sizeof(brov_result));
    } else {
        // the gathered pairs are reduced on rank 0 and the winner's (owner rank, global index, cost) comes back through the mailbox; its
        // whole record is already in the owner's own mailbox (group_pack_kernel) when the owner is a rank of this process
        if (int rc = deliver(g, [&](GroupRank& r, int32_t seq) { hipLaunchKernelGGL(group_pairs_kernel, dim3(1), dim3(64), 0, r.st, r.pairs, g->W, r.mail, seq); }))
            return rc;
        if (mail->owner >= 0) {
            *best_index = mail->slot;
            if (best) {
                std::memset(best, 0, sizeof(*best));
                const int d = mail->owner - g->r0;
                if (d >= 0 && d < g->n) {   // the winner lives in this process: its whole record
                    std::memcpy(best, &g->ranks[d].pmail->rec, sizeof(brov_result));
                } else {                    // ... in another process (one process per GPU): the pair carries its cost only
                    best->cost = mail->rec.cost; best->status = BROV_STATUS_SUCCESS;
                }
            }
        }
    }
    return BROV_OK;
}

int brov_group_get_results_host(brov_group* g, brov_result* res) {
    if (!g || !res) return BROV_ERR_ARG;
    if (g->last_mode != BROV_GATHER_RECORDS) { g_gerr = "brov_group_get_results_host: needs a BROV_GATHER_RECORDS gather"; return BROV_ERR_ARG; }
    if (int rc = brov_group_synchronize(g)) return rc;
    DeviceKeeper keep;
    HIPCHK(hipSetDevice(g->ranks[0].dev));
    for (int r = 0; r < g->W; r++)   // strip the padding slots of uneven shards
        HIPCHK(hipMemcpy(res + g->lo[r], g->ranks[0].gathered + (size_t)r * g->Bmax, (size_t)g->cnt[r] * sizeof(brov_result), hipMemcpyDeviceToHost));
    return BROV_OK;
}
const brov_result* brov_group_gathered_device(const brov_group* g, int rank) { return (g && rank >= 0 && rank < g->n) ? g->ranks[rank].gathered : nullptr; }
int brov_group_slots_per_rank(const brov_group* g) { return g ? g->Bmax : 0; }

int brov_group_last_seconds(brov_group* g, double* solve, double* gather, double* select) {
    if (!g || !g->timing || !g->ev_solve) { g_gerr = "brov_group_last_seconds: no timed solve yet (timing must be on before brov_group_solve)"; return BROV_ERR_ARG; }
    double ts = 0, tg = 0, tsel = 0;
    DeviceKeeper keep;
    for (GroupRank& r : g->ranks) {
        HIPCHK(hipSetDevice(r.dev));
        float a = 0, b = 0;
        HIPCHK(hipEventSynchronize(r.ev[1]));
        HIPCHK(hipEventElapsedTime(&a, r.ev[0], r.ev[1]));
        if (g->last_mode >= 0 && g->ev_gather) { HIPCHK(hipEventSynchronize(r.ev[2])); HIPCHK(hipEventElapsedTime(&b, r.ev[1], r.ev[2])); }
        if (a * 1e-3 > ts) ts = a * 1e-3;
        if (b * 1e-3 > tg) tg = b * 1e-3;
    }
    if (g->last_mode >= 0 && g->ev_sel && g->ev_gather) {   // (an event that was never recorded makes hipEventElapsedTime fail, and the failure would stay
        float c = 0;                        // behind as the thread's "last error" for the next hipGetLastError of an unrelated call)
        GroupRank& r0 = g->ranks[0];
        HIPCHK(hipSetDevice(r0.dev));
        HIPCHK(hipEventSynchronize(r0.ev[3]));
        HIPCHK(hipEventElapsedTime(&c, r0.ev[2], r0.ev[3]));
        tsel = c * 1e-3;
    }
    if (solve) *solve = ts;
    if (gather) *gather = tg;
    if (select) *select = tsel;
    return BROV_OK;
}

}  // extern "C"
