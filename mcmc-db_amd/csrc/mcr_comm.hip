// mcr_comm.hip -- multi-GPU: the RCCL communicator, the mcr_comm_* entries of libmcmcref_hip.so's C ABI.
// Of the rest of the library it uses the context and its error path alone (mcr_host.hpp); it launches no kernel.
#include "mcr_host.hpp"

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <memory>
#include <new>
#include <thread>

#include "mcr_comm.hpp"

using namespace mcr::host;

extern "C" {

struct mcr_comm {
    mcr_ctx* ctx = nullptr;
    ncclComm_t nccl = nullptr;
    hipStream_t stream = nullptr;
    int world = 1, rank = 0;
    DevBuf dbuf;                                  // device staging (send block + receive blocks)
    bool dead = false;                            // aborted after a deadline or an asynchronous error
    double timeout_s = 300.0;                     // MCR_COMM_TIMEOUT_S
};

namespace {
int comm_fail(mcr_ctx* ctx, const char* what, ncclResult_t r)
{
    mcr::comm::Api* a = mcr::comm::api();
    return fail(ctx, MCR_ECOMM, "%s failed: %s", what, a ? a->GetErrorString(r) : "RCCL error");
}

// A DEADLINE ON EVERY COLLECTIVE.  The ranks are separate processes; one that dies after the
// rendezvous (the reference's generate loop carries on past a failed recipe, src/mcmc_ref/generate.py:77-96 -- a sharded
// one must at least not hang on it) would leave its peers inside ncclCommInitRank / ncclAllGather for ever.  So:
//   * ncclCommInitRank runs on a helper thread and the caller only watches the clock (a rank whose peers never come does
//     not return from it, and on RCCL 2.27.7 neither does an abort of it);
//   * the collectives are enqueued on the communicator's stream as usual (the RCCL call returns once its kernel is in the
//     stream) and the wait for that stream is a poll of hipStreamQuery + ncclCommGetAsyncError against
//     MCR_COMM_TIMEOUT_S (default 300 s; the first init of a node can take tens of seconds) instead of a
//     hipStreamSynchronize.  Only then is the result copied to the caller's (pageable) buffer: that copy would block
//     the host behind a stuck collective;
//   * on expiry, or on an asynchronous RCCL error, the communicator is aborted (ncclCommAbort, itself bounded: it tears
//     down the stuck kernel and the proxy), marked dead, and the call returns MCR_ECOMM naming the call, the rank and the
//     time; every later call on it fails at once.
// The communicator itself is the ordinary BLOCKING one (what every RCCL application runs).  A non-blocking one and a mode
// without deadlines were built and removed.
using comm_clock = std::chrono::steady_clock;

// ncclCommAbort with a bound of its own: measured on RCCL 2.27.7, aborting a communicator whose ncclCommInitRank is still
// waiting for a peer does not return (it joins the bootstrap it is meant to cancel).  The abort therefore runs on a helper
// thread that this call waits for at most kAbortGraceS; a helper that has not come back by then is left behind (detached:
// it owns nothing but the communicator handle, which nobody uses again) -- the caller gets its error either way.
constexpr double kAbortGraceS = 5.0;
void bounded_abort(ncclComm_t nccl)
{
    mcr::comm::Api* a = mcr::comm::api();
    if (!a || !nccl) return;
    auto done = std::make_shared<std::atomic<int>>(0);
    std::thread([a, nccl, done]() { a->CommAbort(nccl); done->store(1, std::memory_order_release); }).detach();
    const comm_clock::time_point t0 = comm_clock::now();
    while (!done->load(std::memory_order_acquire) && std::chrono::duration<double>(comm_clock::now() - t0).count() < kAbortGraceS)
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
}

int comm_abort(mcr_comm* c, const char* what, const char* why)
{
    bounded_abort(c->nccl);
    c->nccl = nullptr;
    c->dead = true;
    return fail(c->ctx, MCR_ECOMM, "%s: rank %d of %d gave up: %s (MCR_COMM_TIMEOUT_S = %g s); the communicator was aborted",
                what, c->rank, c->world, why, c->timeout_s);
}

// Waits until the work on the communicator's stream has finished, the communicator reports an asynchronous error, or
// the deadline passes.
int comm_wait(mcr_comm* c, const char* what)
{
    mcr::comm::Api* a = mcr::comm::api();
    const comm_clock::time_point t0 = comm_clock::now();
    for (int spins = 0;; ) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return MCR_OK;
        if (q != hipErrorNotReady) return fail(c->ctx, MCR_EHIP, "%s: hipStreamQuery failed: %s", what, hipGetErrorString(q));
        ncclResult_t st = ncclSuccess;
        if (a->CommGetAsyncError(c->nccl, &st) == ncclSuccess && st != ncclSuccess && st != ncclInProgress) {
            char why[160];
            snprintf(why, sizeof why, "asynchronous RCCL error: %s", a->GetErrorString(st));
            return comm_abort(c, what, why);
        }
        if (std::chrono::duration<double>(comm_clock::now() - t0).count() > c->timeout_s)
            return comm_abort(c, what, "the collective did not complete before the deadline (a peer is gone or stuck)");
        if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// The one path of both collectives: `in_bytes` from `in` are uploaded to the front of the staging buffer, `rccl` issues
// the collective on the communicator's stream with (staging, staging + out_at), and the `out_bytes` at out_at are
// copied to `out` -- after the bounded wait, so a timeout or an RCCL error never writes the caller's buffer.
int comm_collective(mcr_comm* c, const char* what, bool args_ok, const double* in, size_t in_bytes, double* out,
                    size_t out_at, size_t out_bytes, const std::function<ncclResult_t(void*, void*)>& rccl)
{
    mcr_ctx* ctx = c->ctx;
    if (c->dead) return fail(ctx, MCR_ECOMM, "%s: the communicator of rank %d was aborted by an earlier failure", what, c->rank);
    if (!args_ok) return fail(ctx, MCR_EINVAL, "bad argument");
    if (in_bytes == 0) return MCR_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc = c->dbuf.reserve(ctx, out_at + out_bytes);      // (a collective returns with the communicator's stream idle, or dead)
    if (rc) return rc;
    char* d = c->dbuf.as<char>();
    HIP_TRY(ctx, hipMemcpyAsync(d, in, in_bytes, hipMemcpyHostToDevice, c->stream));
    const ncclResult_t r = rccl(d, d + out_at);
    if (r != ncclSuccess) return comm_fail(ctx, what, r);
    rc = comm_wait(c, what);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(out, d + out_at, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(ctx, hipStreamSynchronize(c->stream));
    return MCR_OK;
}
}  // namespace

int mcr_comm_unique_id(void* id, size_t len)
{
    if (!id || len < MCR_COMM_ID_BYTES) return fail(nullptr, MCR_EINVAL, "id buffer must hold %d bytes", MCR_COMM_ID_BYTES);
    mcr::comm::Api* a = mcr::comm::api();
    if (!a) return fail(nullptr, MCR_ECOMM, "librccl could not be loaded: %s", mcr::comm::api_why());
    static_assert(sizeof(ncclUniqueId) == MCR_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId uid;
    const ncclResult_t r = a->GetUniqueId(&uid);
    if (r != ncclSuccess) return comm_fail(nullptr, "ncclGetUniqueId", r);
    memcpy(id, &uid, sizeof uid);
    return MCR_OK;
}

int mcr_comm_init(mcr_ctx* ctx, const void* id, int world, int rank, mcr_comm** out)
{
    if (!ctx) return fail(nullptr, MCR_EINVAL, "ctx is NULL");
    if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(ctx, MCR_EINVAL, "bad communicator arguments (world %d, rank %d)", world, rank);
    *out = nullptr;
    mcr::comm::Api* a = mcr::comm::api();
    if (!a) return fail(ctx, MCR_ECOMM, "librccl could not be loaded: %s", mcr::comm::api_why());
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    mcr_comm* c = new (std::nothrow) mcr_comm();
    if (!c) return fail(ctx, MCR_ENOMEM, "out of host memory");
    c->ctx = ctx; c->world = world; c->rank = rank;
    if (const char* env = getenv("MCR_COMM_TIMEOUT_S")) { const double v = atof(env); if (v > 0.0) c->timeout_s = v; }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(ctx, MCR_EHIP, "hipStreamCreate failed: %s", hipGetErrorString(e)); }
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof uid);
    // Collective: every rank of the world calls it.  The init runs on a helper thread and THIS thread only watches the
    // clock: on RCCL 2.27.7 neither the init of a rank whose peers never come nor an abort of it is guaranteed to return,
    // and the caller must get its error anyway.
    struct InitJob {
        std::atomic<int> state{0};                 // 1: finished (r says how)
        std::atomic<ncclComm_t> nccl{nullptr};
        ncclResult_t r = ncclSuccess;
    };
    auto job = std::make_shared<InitJob>();
    const int dev = ctx->device;
    std::thread([a, job, dev, world, uid, rank]() {
        hipSetDevice(dev);
        ncclComm_t h = nullptr;
        job->r = a->CommInitRank(&h, world, uid, rank);          // returns when every rank has arrived -- or never
        job->nccl.store(h, std::memory_order_release);
        job->state.store(1, std::memory_order_release);
    }).detach();
    const comm_clock::time_point t0 = comm_clock::now();
    int spins = 0;
    while (!job->state.load(std::memory_order_acquire) &&
           std::chrono::duration<double>(comm_clock::now() - t0).count() <= c->timeout_s)
        if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(100));
    int rc = MCR_OK;
    if (!job->state.load(std::memory_order_acquire)) {
        bounded_abort(job->nccl.load(std::memory_order_acquire));   // nullptr unless the init returned just now
        rc = fail(ctx, MCR_ECOMM, "ncclCommInitRank: rank %d of %d gave up: a peer did not arrive before the deadline "
                  "(MCR_COMM_TIMEOUT_S = %g s); the communicator was aborted", rank, world, c->timeout_s);
    } else if (job->r != ncclSuccess) rc = comm_fail(ctx, "ncclCommInitRank", job->r);
    else if (!job->nccl.load()) rc = fail(ctx, MCR_ECOMM, "ncclCommInitRank returned no communicator");
    if (rc) { hipStreamDestroy(c->stream); delete c; return rc; }
    c->nccl = job->nccl.load();
    *out = c;
    return MCR_OK;
}

void mcr_comm_free(mcr_comm* c)
{
    if (!c) return;
    hipSetDevice(c->ctx->device);
    if (c->nccl && !c->dead && comm_wait(c, "mcr_comm_free") == MCR_OK) mcr::comm::api()->CommDestroy(c->nccl);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int mcr_comm_world(const mcr_comm* c) { return c ? c->world : -1; }
int mcr_comm_rank(const mcr_comm* c) { return c ? c->rank : -1; }
int mcr_comm_has_deadline(const mcr_comm* c) { return c ? 1 : 0; }

// THE collective of the path: every rank contributes `count` doubles, every rank receives world * count doubles in
// rank order (ncclAllGather over xGMI).  Host pointers; staged through a small device buffer on the communicator's stream.
int mcr_comm_all_gather(mcr_comm* c, const double* send, int64_t count, double* recv)
{
    if (!c) return fail(nullptr, MCR_EINVAL, "comm is NULL");
    const size_t sb = (size_t)count * 8;
    return comm_collective(c, "ncclAllGather", count >= 0 && (count == 0 || (send && recv)), send, sb, recv,
                           align_up(sb, 256), sb * (size_t)c->world, [c, count](void* d_send, void* d_recv) {
                               return mcr::comm::api()->AllGather(d_send, d_recv, (size_t)count, ncclDouble, c->nccl, c->stream);
                           });
}

// Element-wise reduction of n host doubles over the ranks, in place (op: 0 sum, 1 max, 2 min): the bench's
// max-over-ranks clock and "every rank validated" flag, and (n = 1) a barrier.
int mcr_comm_all_reduce(mcr_comm* c, double* vals, int64_t n, int op)
{
    if (!c) return fail(nullptr, MCR_EINVAL, "comm is NULL");
    const size_t b = (size_t)n * 8;
    return comm_collective(c, "ncclAllReduce", n >= 0 && (n == 0 || vals) && op >= 0 && op <= 2, vals, b, vals, 0, b,
                           [c, n, op](void* d_in, void* d_out) {
                               const ncclRedOp_t ops[3] = {ncclSum, ncclMax, ncclMin};
                               return mcr::comm::api()->AllReduce(d_in, d_out, (size_t)n, ncclDouble, ops[op], c->nccl, c->stream);
                           });
}

int mcr_comm_barrier(mcr_comm* c)
{
    if (!c) return fail(nullptr, MCR_EINVAL, "comm is NULL");
    for (const mcr_ctx::Lane& l : c->ctx->lanes) if (l.stream) HIP_TRY(c->ctx, hipStreamSynchronize(l.stream));
    double one = 1.0;
    return mcr_comm_all_reduce(c, &one, 1, 0);
}

}  // extern "C"
