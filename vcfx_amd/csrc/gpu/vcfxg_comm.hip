// vcfxg_comm.hip -- rank cliques: the count all-reduce of the in-process multi-GPU drop-in
// RCCL comes from librccl at run time (dlopen: a single-GPU process never loads it).  rccl.h is
// included for its declarations only: the function pointer types and the enum values below are
// checked against it at compile time (no link dependency).
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <condition_variable>
#include <mutex>

#include "vcfxg_ctx.h"

namespace {
typedef decltype(&ncclCommInitAll) nccl_init_all_f;
typedef decltype(&ncclAllReduce) nccl_allreduce_f;
typedef decltype(&ncclCommDestroy) nccl_destroy_f;
static_assert(ncclUint64 == 5 && ncclSum == 0 && ncclSuccess == 0, "rccl.h enum values");
constexpr size_t kCommSlots = 64;  // u64 values per all-reduce
}  // namespace

struct vcfxg_comm {
    int n = 0;
    std::vector<vcfxg_ctx *> ctx;
    // RCCL
    void *lib = nullptr;
    nccl_allreduce_f allreduce = nullptr;
    nccl_destroy_f destroy = nullptr;
    std::vector<ncclComm_t> comms;
    std::vector<uint64_t *> dbuf;  // per rank: kCommSlots u64 on its device
    // host side: every all-reduce is first a host reduction + vote of all ranks (the RCCL result
    // is checked against it, and no rank enters the collective unless every rank staged its values)
    std::mutex mu;
    std::condition_variable cv;
    uint64_t gen = 0;
    int arrived = 0, failed = 0;
    bool result_failed = false;
    std::vector<uint64_t> acc, result;
    uint64_t rccl_calls = 0, rccl_mismatch = 0;
};

extern "C" {

int vcfxg_comm_init(vcfxg_ctx *const *ctxs, int n, vcfxg_comm **out) {
    if (!ctxs || n < 1 || !out) return VCFXG_E_ARG;
    vcfxg_comm *c = new vcfxg_comm;
    c->n = n;
    c->ctx.assign(ctxs, ctxs + n);
    std::vector<int> dev(n);
    bool distinct = n > 1;
    for (int r = 0; r < n; r++) {
        if (!ctxs[r]) {
            delete c;
            return VCFXG_E_ARG;
        }
        dev[r] = ctxs[r]->device;
        for (int q = 0; q < r; q++) distinct = distinct && dev[q] != dev[r];
    }
    // RCCL over n distinct devices; VCFX_RCCL=1 also forms a one-rank clique (a one-GPU box runs
    // the whole RCCL path: init, the collective on the rank's stream, destroy); VCFX_RCCL=0 never.
    // RCCL cannot put two ranks on one device, so ranks sharing one reduce on the host.
    const char *e = getenv("VCFX_RCCL");
    const bool want = (distinct && !(e && e[0] == '0')) || (n == 1 && e && e[0] == '1');
    if (want) {
        c->lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!c->lib) c->lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        nccl_init_all_f init = c->lib ? (nccl_init_all_f)dlsym(c->lib, "ncclCommInitAll") : nullptr;
        c->allreduce = c->lib ? (nccl_allreduce_f)dlsym(c->lib, "ncclAllReduce") : nullptr;
        c->destroy = c->lib ? (nccl_destroy_f)dlsym(c->lib, "ncclCommDestroy") : nullptr;
        c->comms.assign(n, nullptr);
        if (!init || !c->allreduce || !c->destroy || init(c->comms.data(), n, dev.data()) != ncclSuccess) {
            if (c->lib) dlclose(c->lib);
            c->lib = nullptr;
            c->allreduce = nullptr;
            c->comms.clear();
            ctxs[0]->err = "vcfxg_comm_init: RCCL clique over " + std::to_string(n) + " devices failed";
            delete c;
            return VCFXG_E_HIP;
        }
        c->dbuf.assign(n, nullptr);
        for (int r = 0; r < n; r++) {
            if (hipSetDevice(dev[r]) != hipSuccess || hipMalloc((void **)&c->dbuf[r], kCommSlots * 8) != hipSuccess) {
                ctxs[r]->err = "vcfxg_comm_init: no device buffer for the all-reduce";
                vcfxg_comm_destroy(c);
                return VCFXG_E_HIP;
            }
        }
    }
    c->acc.assign(kCommSlots, 0);
    c->result.assign(kCommSlots, 0);
    *out = c;
    return VCFXG_OK;
}

int vcfxg_comm_uses_rccl(const vcfxg_comm *c) { return c && c->allreduce ? 1 : 0; }

int vcfxg_comm_rccl_stats(vcfxg_comm *c, uint64_t *calls, uint64_t *mismatches) {
    if (!c) return VCFXG_E_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (calls) *calls = c->rccl_calls;
    if (mismatches) *mismatches = c->rccl_mismatch;
    return VCFXG_OK;
}

int vcfxg_comm_allreduce_u64(vcfxg_comm *c, int rank, uint64_t *vals, size_t count) {
    if (!c || rank < 0 || rank >= c->n || (!vals && count) || count > kCommSlots) return VCFXG_E_ARG;
    vcfxg_ctx *x = c->ctx[rank];
    // 1. stage the values on the rank's device (RCCL); a rank whose device call fails votes "no"
    bool ok = true;
    if (c->allreduce) {
        ok = hipSetDevice(x->device) == hipSuccess &&
             hipMemcpyAsync(c->dbuf[rank], vals, 8 * count, hipMemcpyHostToDevice, x->stream) == hipSuccess &&
             hipStreamSynchronize(x->stream) == hipSuccess;
        if (!ok) x->err = "vcfxg_comm_allreduce_u64: staging the values on the device failed";
    }
    // 2. host reduction + vote: the last rank to arrive publishes the sums of this generation
    std::vector<uint64_t> host(count);
    bool any_failed;
    {
        std::unique_lock<std::mutex> lk(c->mu);
        const uint64_t g = c->gen;
        for (size_t k = 0; k < count; k++) c->acc[k] += vals[k];
        if (!ok) c->failed++;
        if (++c->arrived == c->n) {
            c->result = c->acc;
            c->result_failed = c->failed != 0;
            std::fill(c->acc.begin(), c->acc.end(), 0);
            c->arrived = c->failed = 0;
            c->gen++;
            c->cv.notify_all();
        } else {
            c->cv.wait(lk, [&] { return c->gen != g; });
        }
        std::copy(c->result.begin(), c->result.begin() + (long)count, host.begin());
        any_failed = c->result_failed;
    }
    if (!c->allreduce) {
        std::copy(host.begin(), host.end(), vals);
        return VCFXG_OK;
    }
    if (any_failed) {  // no rank enters the collective; the host sums stand, the failure is reported
        std::copy(host.begin(), host.end(), vals);
        if (ok) x->err = "vcfxg_comm_allreduce_u64: another rank failed to stage its values";
        return VCFXG_E_HIP;
    }
    // 3. RCCL over the devices (xGMI), on the rank's own stream; checked against the host sums
    std::vector<uint64_t> dv(count);
    if (c->allreduce(c->dbuf[rank], c->dbuf[rank], count, ncclUint64, ncclSum, c->comms[rank], x->stream) !=
        ncclSuccess) {
        x->err = "ncclAllReduce failed";
        std::copy(host.begin(), host.end(), vals);
        return VCFXG_E_HIP;
    }
    if (hipMemcpyAsync(dv.data(), c->dbuf[rank], 8 * count, hipMemcpyDeviceToHost, x->stream) != hipSuccess ||
        hipStreamSynchronize(x->stream) != hipSuccess) {
        x->err = "vcfxg_comm_allreduce_u64: reading the RCCL sums back failed";
        std::copy(host.begin(), host.end(), vals);
        return VCFXG_E_HIP;
    }
    const bool same = dv == host;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->rccl_calls++;
        if (!same) c->rccl_mismatch++;
    }
    std::copy(host.begin(), host.end(), vals);
    if (!same) {
        x->err = "vcfxg_comm_allreduce_u64: the RCCL sums differ from the host reduction";
        return VCFXG_E_HIP;
    }
    return VCFXG_OK;
}

void vcfxg_comm_destroy(vcfxg_comm *c) {
    if (!c) return;
    for (size_t r = 0; r < c->comms.size(); r++)
        if (c->comms[r] && c->destroy) c->destroy(c->comms[r]);
    for (size_t r = 0; r < c->dbuf.size(); r++)
        if (c->dbuf[r]) {
            (void)hipSetDevice(c->ctx[r]->device);
            (void)hipFree(c->dbuf[r]);
        }
    // (librccl stays loaded: its teardown threads may still be unwinding)
    delete c;
}

}  // extern "C"
