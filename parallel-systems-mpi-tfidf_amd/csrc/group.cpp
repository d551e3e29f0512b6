/*
 * group.cpp — several GPU shards driven by one process (the drop-in for
 * `mpirun -np P ./TFIDF`, TFIDF.c:82-92,125-130), and the two rank transports of
 * xport.h.
 *
 *   tfidf_group_open   opens one context per rank (rank r on devices[r]) and connects
 *                      them: ncclCommInitAll when every rank has its own GPU (RCCL over
 *                      xGMI), the in-process LocalXport when a device carries several
 *                      ranks (or TFIDF_GROUP_LOCAL is asked for).
 *   tfidf_group_run    one host thread per rank, each runs tfidf_run on its shard; the
 *                      ranks meet only inside the DF exchange (engine.cpp).
 *   tfidf_group_write_output
 *                      every rank formats its lines on its GPU (in parallel), then the
 *                      texts are written in rank order — shards are contiguous ranges of
 *                      the "docN@" order, so this is the reference's gather + qsort
 *                      (TFIDF.c:253-273) without either.
 */
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/tfidf.h"
#include "kernels.h"
#include "xport.h"
#include "devbuf.h"
#include "comm_rank.h"
#include "comm_init.h"

namespace {

/* ------------------------------------------------------------------ RCCL -- */

/* RCCL behind comm_rank.h's abort protocol: communicators are non-blocking, every call and
 * every wait for a collective's kernels is a poll that also watches the clique's `aborted`
 * flag, and each rank only ever aborts its own communicator (from its own thread). */
struct RcclB {
    using Comm = ncclComm_t;
    static int async(Comm c) {
        ncclResult_t st = ncclSuccess;
        if (ncclCommGetAsyncError(c, &st) != ncclSuccess) return TFIDF_E_RCCL;
        return st == ncclInProgress ? 1 : (st == ncclSuccess ? 0 : TFIDF_E_RCCL);
    }
    static void abort(Comm c) { (void)ncclCommAbort(c); }
};
static int nccl_issue(ncclResult_t r) { return r == ncclSuccess ? 0 : (r == ncclInProgress ? 1 : TFIDF_E_RCCL); }

/* Finalizes (non-blocking: all at once, then polled) and destroys the live communicators of
 * one process — a clique's ranks must not be finalized one after the other, since a
 * finalize may wait for the peers'. Communicators that do not finalize within the deadline
 * are aborted. */
static void comms_close(std::vector<ncclComm_t>& comms, int64_t timeout_ms) {
    std::vector<int> st(comms.size(), 0);   /* 1 finalizing, 2 finalized, -1 failed */
    for (size_t r = 0; r < comms.size(); ++r)
        if (comms[r]) st[r] = nccl_issue(ncclCommFinalize(comms[r])) < 0 ? -1 : 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (bool busy = true; busy;) {
        busy = false;
        for (size_t r = 0; r < comms.size(); ++r) {
            if (st[r] != 1) continue;
            const int a = RcclB::async(comms[r]);
            if (a == 1) busy = true;
            else st[r] = a == 0 ? 2 : -1;
        }
        if (busy && timeout_ms > 0 && std::chrono::duration_cast<std::chrono::milliseconds>(
                                          std::chrono::steady_clock::now() - t0).count() > timeout_ms) {
            for (size_t r = 0; r < comms.size(); ++r)
                if (st[r] == 1) st[r] = -1;
            break;
        }
        if (busy) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    for (size_t r = 0; r < comms.size(); ++r) {
        if (!comms[r]) continue;
        if (st[r] == 2) (void)ncclCommDestroy(comms[r]);
        else (void)ncclCommAbort(comms[r]);
        comms[r] = nullptr;
    }
}

/* The communicators of one tfidf_group clique (one process, one host thread per rank).
 * Created together (non-blocking ncclCommInitRankConfig in one group), closed together;
 * during runs rank r's communicator is touched by rank r's thread only. */
struct Clique {
    std::vector<ncclComm_t> comms;
    std::vector<char> dead;                 /* rank r aborted its communicator (written by rank r) */
    std::shared_ptr<CommShared> shared = std::make_shared<CommShared>();
    int64_t timeout_ms = comm_timeout_ms_from_env();
    explicit Clique(int n) : comms((size_t)n, nullptr), dead((size_t)n, 0) {}
    ~Clique() {
        for (size_t r = 0; r < comms.size(); ++r)
            if (dead[r]) comms[r] = nullptr;   /* ncclCommAbort freed it */
        comms_close(comms, timeout_ms);
    }
};

/* polls every communicator of a non-blocking init until it is ready (0), failed or timed out */
static int comms_ready(std::vector<ncclComm_t>& comms, int64_t timeout_ms) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        bool busy = false;
        for (ncclComm_t c : comms) {
            const int a = c ? RcclB::async(c) : TFIDF_E_RCCL;
            if (a < 0) return a;
            busy |= a == 1;
        }
        if (!busy) return TFIDF_OK;
        if (timeout_ms > 0 && std::chrono::duration_cast<std::chrono::milliseconds>(
                                  std::chrono::steady_clock::now() - t0).count() > timeout_ms)
            return TFIDF_E_PEER;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

struct RcclXport final : Xport {
    CommRank<RcclB> cr;                    /* this rank's communicator and the clique's flag */
    std::shared_ptr<Clique> clique;        /* a tfidf_group clique owns the communicator; else this */
    int device = 0;
    DevBuf dwords_buf;   /* 2 (send) + 2 * nranks (recv) */
    ~RcclXport() override {
        if (!clique && !cr.dead && cr.comm) {
            std::vector<ncclComm_t> one{cr.comm};
            comms_close(one, cr.timeout_ms);
        }
    }
    void note_dead() {
        if (clique && cr.dead) clique->dead[rank] = 1;
    }
    /* one RCCL call f(comm) and its completion; TFIDF_E_PEER once the clique was aborted */
    template <class F> int enqueue(F&& f) {
        const int rc = cr.enqueue([&](ncclComm_t c) { return nccl_issue(f(c)); });
        note_dead();
        return rc;
    }
    /* the stream's work (a collective's kernels among it) done, polled; an abort of the
     * clique aborts this rank's communicator, which releases kernels still waiting for a
     * failed peer, and the stream is then drained */
    int wait(hipStream_t s) override {
        const int rc = cr.wait_stream([&] {
            const hipError_t e = hipStreamQuery(s);
            return e == hipSuccess ? 0 : (e == hipErrorNotReady ? 1 : TFIDF_E_HIP);
        });
        (void)hipGetLastError();   /* hipErrorNotReady must not linger as the thread's last error */
        note_dead();
        if (rc) (void)hipStreamSynchronize(s);
        return rc;
    }
    int words(const uint64_t mine[2], uint64_t* all, hipStream_t s) override {
        if (!dwords_buf.p && dwords_buf.exact(16 * (size_t)(nranks + 1))) return TFIDF_E_NOMEM;
        uint64_t* dwords = dwords_buf.as<uint64_t>();
        if (hipMemcpyAsync(dwords, mine, 16, hipMemcpyHostToDevice, s) != hipSuccess) return TFIDF_E_HIP;
        int rc = enqueue([&](ncclComm_t c) { return ncclAllGather(dwords, dwords + 2, 2, ncclUint64, c, s); });
        if (rc) return rc;
        if (hipMemcpyAsync(all, dwords + 2, 16 * (size_t)nranks, hipMemcpyDeviceToHost, s) != hipSuccess)
            return TFIDF_E_HIP;
        return wait(s);
    }
    int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        return enqueue([&](ncclComm_t c) { return ncclAllGather(send, recv, bytes, ncclUint8, c, s); });
    }
    int alltoallv(const void* send, const uint64_t* scnt, void* recv, const uint64_t* rcnt, size_t eb,
                  hipStream_t s) override {
        /* point-to-point pairs in one group: over xGMI every pair of GPUs has its own link */
        return enqueue([&](ncclComm_t c) {
            ncclResult_t r = ncclGroupStart();
            uint64_t so = 0, ro = 0;
            for (int p = 0; p < nranks && r == ncclSuccess; ++p) {
                if (scnt[p]) r = ncclSend((const uint8_t*)send + so * eb, scnt[p] * eb, ncclUint8, p, c, s);
                if (r == ncclSuccess && rcnt[p]) r = ncclRecv((uint8_t*)recv + ro * eb, rcnt[p] * eb, ncclUint8, p, c, s);
                so += scnt[p];
                ro += rcnt[p];
            }
            const ncclResult_t e = ncclGroupEnd();
            return (r != ncclSuccess && r != ncclInProgress) ? r : e;
        });
    }
    int allreduce_u32(uint32_t* buf, size_t n, hipStream_t s) override {
        return enqueue([&](ncclComm_t c) { return ncclAllReduce(buf, buf, n, ncclUint32, ncclSum, c, s); });
    }
    /* this rank failed between collectives: the clique gives up (each peer aborts its own
     * communicator at its next poll), this rank's communicator at once */
    void abort() override {
        cr.fail();
        note_dead();
    }
    const char* name() const override { return "rccl"; }
};

/* -------------------------------------------------------------- in-process -- */

struct Hub {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool poisoned = false;
    std::vector<const void*> ptr;
    std::vector<const void*> ptr2;   /* allreduce: every rank's reduced slice */
    std::vector<int> dev;
    std::vector<uint64_t> w;
    std::vector<uint64_t> sc;   /* alltoallv: rank r's count for peer p at sc[r * n + p] */
    /* returns false when a rank aborted */
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (poisoned) return false;
        const uint64_t g = gen;
        if (++arrived == n) {
            arrived = 0;
            ++gen;
            cv.notify_all();
            return true;
        }
        cv.wait(lk, [&] { return gen != g || poisoned; });
        return gen != g;   /* completed, or released by a poisoning rank */
    }
    void poison() {
        std::lock_guard<std::mutex> lk(mu);
        poisoned = true;
        cv.notify_all();
    }
    /* before a new group run, when no rank is inside the hub: an abort of the previous run
     * does not poison this one */
    void reset() {
        std::lock_guard<std::mutex> lk(mu);
        poisoned = false;
        arrived = 0;
    }
};

struct LocalXport final : Xport {
    Hub* hub = nullptr;
    int device = 0;
    /* every rank on this device (and few enough for one copy list): each collective is one
     * or two kernels reading the peers' buffers directly, instead of one copy per peer */
    bool one_device() const {
        if (nranks > XCOPY_MAX) return false;
        for (int r = 0; r < nranks; ++r)
            if (hub->dev[r] != device) return false;
        return true;
    }
    int words(const uint64_t mine[2], uint64_t* all, hipStream_t s) override {
        (void)s;
        hub->w[2 * rank] = mine[0];
        hub->w[2 * rank + 1] = mine[1];
        if (!hub->barrier()) return TFIDF_E_PEER;
        memcpy(all, hub->w.data(), 16 * (size_t)nranks);
        if (!hub->barrier()) return TFIDF_E_PEER;   /* nobody rewrites w before all have read */
        return TFIDF_OK;
    }
    int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
        /* the send buffer is complete on this stream; peers copy from it after the barrier */
        if (hipStreamSynchronize(s) != hipSuccess) { abort(); return TFIDF_E_HIP; }
        hub->ptr[rank] = send;
        if (!hub->barrier()) return TFIDF_E_PEER;
        int rc = TFIDF_OK;
        if (bytes % 4 == 0 && one_device()) {
            XCopyList l;
            l.n = (uint32_t)nranks;
            l.off[0] = 0;
            for (int r = 0; r < nranks; ++r) {
                l.src[r] = (const uint32_t*)hub->ptr[r];
                l.dst[r] = (uint32_t*)((uint8_t*)recv + (size_t)r * bytes);
                l.off[r + 1] = l.off[r] + bytes / 4;
            }
            if (launch_xcopy(l, s)) rc = TFIDF_E_HIP;
        }
        for (int r = 0; r < nranks && !rc && bytes && !(bytes % 4 == 0 && one_device()); ++r) {
            uint8_t* dst = (uint8_t*)recv + (size_t)r * bytes;
            const hipError_t e = hub->dev[r] == device
                ? hipMemcpyAsync(dst, hub->ptr[r], bytes, hipMemcpyDeviceToDevice, s)
                : hipMemcpyPeerAsync(dst, device, hub->ptr[r], hub->dev[r], bytes, s);
            if (e != hipSuccess) rc = TFIDF_E_HIP;
        }
        if (hipStreamSynchronize(s) != hipSuccess) rc = TFIDF_E_HIP;
        if (rc) { abort(); return rc; }
        /* every rank has copied every send buffer before any of them is reused */
        if (!hub->barrier()) return TFIDF_E_PEER;
        return TFIDF_OK;
    }
    int alltoallv(const void* send, const uint64_t* scnt, void* recv, const uint64_t* rcnt, size_t eb,
                  hipStream_t s) override {
        if (hipStreamSynchronize(s) != hipSuccess) { abort(); return TFIDF_E_HIP; }
        hub->ptr[rank] = send;
        for (int p = 0; p < nranks; ++p) hub->sc[(size_t)rank * nranks + p] = scnt[p];
        if (!hub->barrier()) return TFIDF_E_PEER;
        int rc = TFIDF_OK;
        uint64_t ro = 0;
        const bool fast = eb % 4 == 0 && one_device();
        XCopyList l;
        l.n = 0;
        l.off[0] = 0;
        for (int p = 0; p < nranks && !rc; ++p) {
            /* peer p's segment for this rank starts after its segments for ranks < rank */
            uint64_t so = 0;
            for (int q = 0; q < rank; ++q) so += hub->sc[(size_t)p * nranks + q];
            const uint64_t n = hub->sc[(size_t)p * nranks + rank];
            if (n != rcnt[p]) rc = TFIDF_E_STATE;
            if (!rc && n && fast) {
                l.src[l.n] = (const uint32_t*)((const uint8_t*)hub->ptr[p] + so * eb);
                l.dst[l.n] = (uint32_t*)((uint8_t*)recv + ro * eb);
                l.off[l.n + 1] = l.off[l.n] + n * eb / 4;
                ++l.n;
            } else if (!rc && n) {
                uint8_t* dst = (uint8_t*)recv + ro * eb;
                const uint8_t* src = (const uint8_t*)hub->ptr[p] + so * eb;
                const hipError_t e = hub->dev[p] == device
                    ? hipMemcpyAsync(dst, src, n * eb, hipMemcpyDeviceToDevice, s)
                    : hipMemcpyPeerAsync(dst, device, src, hub->dev[p], n * eb, s);
                if (e != hipSuccess) rc = TFIDF_E_HIP;
            }
            ro += rcnt[p];
        }
        if (!rc && l.n && launch_xcopy(l, s)) rc = TFIDF_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TFIDF_E_HIP;
        if (rc) { abort(); return rc; }
        if (!hub->barrier()) return TFIDF_E_PEER;   /* no send buffer is reused before all copied */
        return TFIDF_OK;
    }
    /* every rank copies all ranks' vectors into its staging area (after a barrier: all are
     * complete), then (after a second barrier: nobody overwrites a vector still being read)
     * sums them into its own */
    DevBuf stage_buf;
    size_t stage_n = 0;
    int allreduce_u32(uint32_t* buf, size_t n, hipStream_t s) override {
        if (!n) return hub->barrier() && hub->barrier() && hub->barrier() ? TFIDF_OK : TFIDF_E_PEER;
        if (one_device()) return allreduce_slices(buf, n, s);
        if (stage_n < n * (size_t)nranks) {
            stage_n = 0;
            if (stage_buf.exact(n * (size_t)nranks * 4)) { abort(); return TFIDF_E_NOMEM; }
            stage_n = n * (size_t)nranks;
        }
        uint32_t* stage = stage_buf.as<uint32_t>();
        if (hipStreamSynchronize(s) != hipSuccess) { abort(); return TFIDF_E_HIP; }
        hub->ptr[rank] = buf;
        if (!hub->barrier()) return TFIDF_E_PEER;
        int rc = TFIDF_OK;
        for (int r = 0; r < nranks && !rc; ++r) {
            const hipError_t e = hub->dev[r] == device
                ? hipMemcpyAsync(stage + (size_t)r * n, hub->ptr[r], n * 4, hipMemcpyDeviceToDevice, s)
                : hipMemcpyPeerAsync(stage + (size_t)r * n, device, hub->ptr[r], hub->dev[r], n * 4, s);
            if (e != hipSuccess) rc = TFIDF_E_HIP;
        }
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TFIDF_E_HIP;
        if (rc) { abort(); return rc; }
        if (!hub->barrier()) return TFIDF_E_PEER;   /* every vector read before any is overwritten */
        if (launch_sum_rows_u32(stage, (uint32_t)nranks, n, buf, s)) { abort(); return TFIDF_E_HIP; }
        if (hipStreamSynchronize(s) != hipSuccess) { abort(); return TFIDF_E_HIP; }
        if (!hub->barrier()) return TFIDF_E_PEER;
        return TFIDF_OK;
    }
    /* one device: a reduce-scatter (rank r sums slice r of every rank's vector into its
     * staging) and an all-gather of the slices back into every vector; 2 launches per rank,
     * ~3n words of traffic instead of R copies of n words and a row sum */
    int allreduce_slices(uint32_t* buf, size_t n, hipStream_t s) {
        const size_t chunk = (n + nranks - 1) / nranks;
        if (stage_n < chunk) {
            stage_n = 0;
            if (stage_buf.exact(chunk * 4)) { abort(); return TFIDF_E_NOMEM; }
            stage_n = chunk;
        }
        uint32_t* stage = stage_buf.as<uint32_t>();
        auto slice = [&](int r, size_t* lo) {
            *lo = chunk * r < n ? chunk * r : n;
            return (chunk * (r + 1) < n ? chunk * (r + 1) : n) - *lo;
        };
        if (hipStreamSynchronize(s) != hipSuccess) { abort(); return TFIDF_E_HIP; }
        hub->ptr[rank] = buf;
        hub->ptr2[rank] = stage;
        if (!hub->barrier()) return TFIDF_E_PEER;
        XCopyList l;
        l.n = (uint32_t)nranks;
        for (int r = 0; r < nranks; ++r) l.src[r] = (const uint32_t*)hub->ptr[r];
        size_t lo;
        const size_t len = slice(rank, &lo);
        int rc = launch_xsum_slice(l, lo, len, stage, s) ? TFIDF_E_HIP : TFIDF_OK;
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TFIDF_E_HIP;
        if (rc) { abort(); return rc; }
        if (!hub->barrier()) return TFIDF_E_PEER;   /* every slice summed: the vectors are free */
        l.off[0] = 0;
        for (int r = 0; r < nranks; ++r) {
            const size_t m = slice(r, &lo);
            l.src[r] = (const uint32_t*)hub->ptr2[r];
            l.dst[r] = buf + lo;
            l.off[r + 1] = l.off[r] + m;
        }
        if (launch_xcopy(l, s)) rc = TFIDF_E_HIP;
        if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = TFIDF_E_HIP;
        if (rc) { abort(); return rc; }
        if (!hub->barrier()) return TFIDF_E_PEER;   /* every slice read before a staging is reused */
        return TFIDF_OK;
    }
    void abort() override { hub->poison(); }
    const char* name() const override { return "local"; }
};

}  // namespace

/* one rank of a process-per-GPU job (tfidf_comm_init): the init runs with a deadline on a
 * helper thread (comm_init.h: RCCL 2.27 blocks the caller in its bootstrap until every rank
 * joined; at most one abandoned helper per process) */
int rccl_init_rank(const void* unique_id, int rank, int nranks, int device, Xport** out) {
    *out = nullptr;
    ncclUniqueId u;
    memcpy(&u, unique_id, sizeof(u));
    const int64_t tmo = comm_timeout_ms_from_env();
    char who[64];
    snprintf(who, sizeof who, "rank %d of %d", rank, nranks);
    ncclComm_t comm = nullptr;
    const int rc = comm_init_with_deadline<RcclB>(
        [u, rank, nranks, device, tmo](ncclComm_t* c) -> int {
            ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
            cfg.blocking = 0;
            if (hipSetDevice(device) != hipSuccess) return TFIDF_E_HIP;
            if (nccl_issue(ncclCommInitRankConfig(c, nranks, u, rank, &cfg)) < 0 || !*c) return TFIDF_E_RCCL;
            std::vector<ncclComm_t> one{*c};
            return comms_ready(one, tmo);
        },
        tmo, &comm, who);
    if (rc) return rc;
    RcclXport* x = new RcclXport();
    x->cr.comm = comm;
    x->cr.timeout_ms = tmo;
    x->rank = rank;
    x->nranks = nranks;
    x->device = device;
    *out = x;
    return TFIDF_OK;
}

struct tfidf_group {
    int n = 0;
    bool local = false;
    std::vector<tfidf_ctx*> ctx;
    Hub* hub = nullptr;
};

extern "C" {

int tfidf_group_open(int nranks, const int* devices, uint32_t flags, tfidf_group** out) {
    if (!out || nranks < 1 || nranks > 1024) return TFIDF_E_INVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return TFIDF_E_NODEV;
    std::vector<int> dev((size_t)nranks);
    for (int r = 0; r < nranks; ++r) {
        dev[r] = devices ? devices[r] : r;
        if (dev[r] < 0 || dev[r] >= ndev) return TFIDF_E_NODEV;
    }
    bool distinct = true;
    for (int a = 0; a < nranks && distinct; ++a)
        for (int b = a + 1; b < nranks; ++b)
            if (dev[a] == dev[b]) { distinct = false; break; }
    tfidf_group* g = new tfidf_group();
    g->n = nranks;
    g->local = !distinct || (flags & TFIDF_GROUP_LOCAL) != 0;
    g->ctx.assign((size_t)nranks, nullptr);
    int rc = TFIDF_OK;
    for (int r = 0; r < nranks && !rc; ++r) rc = tfidf_open(dev[r], &g->ctx[r]);
    if (!rc && nranks > 1 && g->local) {
        g->hub = new Hub();
        g->hub->n = nranks;
        g->hub->ptr.assign((size_t)nranks, nullptr);
        g->hub->ptr2.assign((size_t)nranks, nullptr);
        g->hub->dev = dev;
        g->hub->w.assign(2 * (size_t)nranks, 0);
        g->hub->sc.assign((size_t)nranks * nranks, 0);
        for (int r = 0; r < nranks && !rc; ++r) {
            LocalXport* x = new LocalXport();
            x->hub = g->hub;
            x->rank = r;
            x->nranks = nranks;
            x->device = dev[r];
            rc = tfidf_ctx_attach_xport(g->ctx[r], x);
        }
    } else if (!rc) {
        /* one RCCL communicator per GPU of the clique (a 1-rank group gets one too, so the
         * exchange path is the same at every size), created non-blocking in one group and
         * owned by the clique: an error on one rank makes every rank abort its own */
        auto cl = std::make_shared<Clique>(nranks);
        ncclUniqueId u;
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (ncclGetUniqueId(&u) != ncclSuccess) rc = TFIDF_E_RCCL;
        if (!rc) {
            ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
            cfg.blocking = 0;
            int bad = nccl_issue(ncclGroupStart()) < 0;
            for (int r = 0; r < nranks && !bad; ++r) {
                if (hipSetDevice(dev[r]) != hipSuccess) bad = 1;
                else bad = nccl_issue(ncclCommInitRankConfig(&cl->comms[r], nranks, u, r, &cfg)) < 0;
            }
            if (nccl_issue(ncclGroupEnd()) < 0) bad = 1;
            (void)hipSetDevice(cur);
            if (bad) rc = TFIDF_E_RCCL;
            else rc = comms_ready(cl->comms, cl->timeout_ms);
            if (rc == TFIDF_E_PEER) {   /* timed out: aborted on a helper thread (an abort may wait in the
                                           same bootstrap; comm_init.h) */
                comm_reap_async<RcclB>(cl->comms);
                for (ncclComm_t& c : cl->comms) c = nullptr;
            } else if (rc) {   /* nothing usable: abort what was created */
                for (ncclComm_t& c : cl->comms)
                    if (c) { (void)ncclCommAbort(c); c = nullptr; }
            }
        }
        for (int r = 0; r < nranks && !rc; ++r) {
            RcclXport* x = new RcclXport();
            x->clique = cl;
            x->cr.comm = cl->comms[r];
            x->cr.shared = cl->shared;
            x->cr.timeout_ms = cl->timeout_ms;
            x->rank = r;
            x->nranks = nranks;
            x->device = dev[r];
            rc = tfidf_ctx_attach_xport(g->ctx[r], x);
        }
    }
    if (rc) {
        tfidf_group_close(g);
        return rc;
    }
    *out = g;
    return TFIDF_OK;
}

int tfidf_group_size(const tfidf_group* g) { return g ? g->n : 0; }

tfidf_ctx* tfidf_group_ctx(tfidf_group* g, int rank) {
    return (g && rank >= 0 && rank < g->n) ? g->ctx[rank] : nullptr;
}

int tfidf_group_run(tfidf_group* g, const tfidf_corpus* shards) {
    if (!g || !shards) return TFIDF_E_INVAL;
    std::vector<int> rc((size_t)g->n, TFIDF_OK);
    if (g->hub) g->hub->reset();   /* in-process ranks: a new run starts unpoisoned */
    std::vector<std::thread> th;
    for (int r = 1; r < g->n; ++r) th.emplace_back([&, r] { rc[r] = tfidf_run(g->ctx[r], &shards[r]); });
    rc[0] = tfidf_run(g->ctx[0], &shards[0]);
    for (auto& t : th) t.join();
    /* the first rank's own error; TFIDF_E_PEER only when no rank has a better reason */
    int peer = TFIDF_OK;
    for (int r = 0; r < g->n; ++r) {
        if (rc[r] == TFIDF_E_PEER) peer = TFIDF_E_PEER;
        else if (rc[r]) return rc[r];
    }
    return peer;
}

/* tfidf_prune on every rank at once.  df is global, so min_df / max_df select the same words
 * on every rank; the shards share no term table, which is why there is no cut by max_features
 * over a group (a global cut is left out). */
int tfidf_group_prune(tfidf_group* g, const tfidf_prune_params* params) {
    if (!g || tfidf_prune_check(params) != TFIDF_OK || params->max_features != 0u) return TFIDF_E_INVAL;
    std::vector<int> rc((size_t)g->n, TFIDF_OK);
    std::vector<std::thread> th;
    for (int r = 1; r < g->n; ++r) th.emplace_back([&, r] { rc[r] = tfidf_prune(g->ctx[r], params); });
    rc[0] = tfidf_prune(g->ctx[0], params);
    for (auto& t : th) t.join();
    for (int r = 0; r < g->n; ++r)
        if (rc[r]) return rc[r];
    return TFIDF_OK;
}

/* tfidf_reweight on every rank at once.  N and df are global and a document's pairs live in one
 * shard, so every shard computes what a single shard would. */
int tfidf_group_reweight(tfidf_group* g, const tfidf_weighting* params) {
    if (!g || tfidf_weighting_check(params) != TFIDF_OK) return TFIDF_E_INVAL;
    std::vector<int> rc((size_t)g->n, TFIDF_OK);
    std::vector<std::thread> th;
    for (int r = 1; r < g->n; ++r) th.emplace_back([&, r] { rc[r] = tfidf_reweight(g->ctx[r], params); });
    rc[0] = tfidf_reweight(g->ctx[0], params);
    for (auto& t : th) t.join();
    for (int r = 0; r < g->n; ++r)
        if (rc[r]) return rc[r];
    return TFIDF_OK;
}

int tfidf_group_write_output(tfidf_group* g, const char* path) {
    if (!g || !path) return TFIDF_E_INVAL;
    std::vector<int> rc((size_t)g->n, TFIDF_OK);
    std::vector<uint64_t> nb((size_t)g->n, 0);
    {   /* every GPU formats its shard's lines at once */
        std::vector<std::thread> th;
        for (int r = 1; r < g->n; ++r) th.emplace_back([&, r] { rc[r] = tfidf_format(g->ctx[r], &nb[r]); });
        rc[0] = tfidf_format(g->ctx[0], &nb[0]);
        for (auto& t : th) t.join();
    }
    for (int r = 0; r < g->n; ++r)
        if (rc[r]) return rc[r];
    for (int r = 0; r < g->n; ++r) {
        const int e = tfidf_write_output_gpu(g->ctx[r], path, r > 0);
        if (e) return e;
    }
    return TFIDF_OK;
}

/* Every rank ranks its own shard (tfidf_query is local to a context), one host thread per
 * rank as in tfidf_group_run; the rows are merged here by (score descending, document id
 * ascending).  The shards partition the documents, so a document of the global top-k is in
 * its shard's top-k and the merge is exact. */
static int group_query(tfidf_group* g, const tfidf_queries* queries, uint32_t k, tfidf_hits* out, const Bm25Call* bm,
                       const ClausePlan* cl = nullptr) {
    if (!g || (!queries && !cl) || !out) return TFIDF_E_INVAL;
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_hits> part((size_t)R);
    std::vector<std::vector<uint8_t>> found((size_t)R);
    std::vector<std::vector<uint64_t>> foff((size_t)R);
    for (tfidf_hits& h : part) memset(&h, 0, sizeof(h));
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r)
            th.emplace_back([&, r] { rc[r] = tfidf_ctx_query(g->ctx[r], queries, k, &part[r], &found[r], &foff[r], bm, cl); });
        rc[0] = tfidf_ctx_query(g->ctx[0], queries, k, &part[0], &found[0], &foff[0], bm, cl);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    const uint32_t nq = cl ? cl->nqueries : queries->nqueries;
    tfidf_hits m;
    memset(&m, 0, sizeof(m));
    if (!err) {
        m.nqueries = nq;
        m.k = k;
        m.nhits = (uint32_t*)calloc((size_t)nq + 1, 4);
        m.nmatch = (uint64_t*)calloc((size_t)nq + 1, 8);
        m.nterms_found = (uint32_t*)calloc((size_t)nq + 1, 4);
        m.doc = (uint32_t*)calloc((size_t)nq * k + 1, 4);
        m.score = (double*)calloc((size_t)nq * k + 1, 8);
        if (!m.nhits || !m.nmatch || !m.nterms_found || !m.doc || !m.score) err = TFIDF_E_NOMEM;
    }
    for (uint32_t q = 0; q < nq && !err; ++q) {
        for (uint64_t x = foff[0][q]; x < foff[0][q + 1]; ++x) {   /* the same term numbering on every rank */
            bool any = false;
            for (int r = 0; r < R; ++r) any = any || found[r][x];
            m.nterms_found[q] += any;
        }
        std::vector<size_t> at((size_t)R, 0);   /* R-way merge of the ranks' ordered rows */
        uint32_t n = 0;
        for (int r = 0; r < R; ++r) m.nmatch[q] += part[r].nmatch[q];
        while (n < k) {
            int best = -1;
            uint64_t bs = 0;
            uint32_t bd = 0;
            for (int r = 0; r < R; ++r) {
                if (at[r] >= part[r].nhits[q]) continue;
                uint64_t sb;
                memcpy(&sb, &part[r].score[(size_t)q * k + at[r]], 8);   /* scores >= +0.0: the bits order like the values */
                const uint32_t d = part[r].doc[(size_t)q * k + at[r]];
                if (best < 0 || sb > bs || (sb == bs && d < bd)) { best = r; bs = sb; bd = d; }
            }
            if (best < 0) break;
            m.doc[(size_t)q * k + n] = bd;
            memcpy(&m.score[(size_t)q * k + n], &bs, 8);
            ++at[best];
            ++n;
        }
        m.nhits[q] = n;
    }
    for (tfidf_hits& h : part) tfidf_hits_free(&h);
    if (err) {
        tfidf_hits_free(&m);
        memset(out, 0, sizeof(*out));
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

int tfidf_group_query(tfidf_group* g, const tfidf_queries* queries, uint32_t k, tfidf_hits* out) {
    return group_query(g, queries, k, out, nullptr);
}

/* BM25 over every shard: with avgdl = 0 the ranks' L and n are summed here (exact integers,
 * one division) and every rank scores with the same avgdl; df and N are the run's global
 * ones, so a document's score is the single-shard run's and the merge is exact. */
static int group_avgdl(tfidf_group* g, Bm25Call* bm) {
    if (bm->avgdl > 0.0) return TFIDF_OK;
    uint64_t L = 0, n = 0;
    for (int r = 0; r < g->n; ++r) {
        uint64_t l = 0, m = 0;
        const int rc = tfidf_ctx_bm25_lengths(g->ctx[r], &l, &m);
        if (rc) return rc;
        L += l;
        n += m;
    }
    if (L) bm->avgdl = (double)L / (double)n;   /* L = 0: no rank has a pair, every row is empty */
    return TFIDF_OK;
}

int tfidf_group_query_bm25(tfidf_group* g, const tfidf_queries* queries, uint32_t k, const tfidf_bm25_params* params,
                           tfidf_hits* out) {
    if (!g || !queries || !out) return TFIDF_E_INVAL;
    Bm25Call bm{};
    int rc = tfidf_bm25_params_check(params, &bm);
    if (rc) return rc;
    rc = group_avgdl(g, &bm);
    if (rc) return rc;
    return group_query(g, queries, k, out, &bm);
}

/* Clauses over every shard: the conditions are decided per document and the shards partition
 * the documents, so the merge of tfidf_group_query is exact here too.  A must term that one
 * shard's vocabulary lacks drops the query on that shard alone: none of its documents holds it. */
int tfidf_group_query_clauses(tfidf_group* g, const tfidf_clauses* clauses, uint32_t k, tfidf_hits* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!g || !clauses || !out) return TFIDF_E_INVAL;
    ClausePlan plan{};
    Bm25Call bm{};
    bool has_bm = false;
    int rc = tfidf_clause_plan(clauses, &plan, &bm, &has_bm);
    if (rc) return rc;
    if (has_bm) {
        rc = group_avgdl(g, &bm);
        if (rc) return rc;
    }
    return group_query(g, nullptr, k, out, has_bm ? &bm : nullptr, &plan);
}

/* Every rank selects on its own host thread (tfidf_top_terms is local to a context).  NULL
 * list: the ranks' rows are concatenated in rank order.  Id list: every rank looks up every
 * id and row r is taken from the first rank that holds it.  pos and pair are moved by the
 * documents and pairs of the ranks before the holder. */
int tfidf_group_top_terms(tfidf_group* g, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_doc_terms* out) {
    if (!g || !out) return TFIDF_E_INVAL;
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_doc_terms> part((size_t)R);
    for (tfidf_doc_terms& p : part) memset(&p, 0, sizeof(p));
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r) th.emplace_back([&, r] { rc[r] = tfidf_top_terms(g->ctx[r], doc_ids, ndocs, k, &part[r]); });
        rc[0] = tfidf_top_terms(g->ctx[0], doc_ids, ndocs, k, &part[0]);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    /* where each rank's documents and pairs start in the concatenated output */
    std::vector<uint64_t> doc0((size_t)R + 1, 0), pair0((size_t)R + 1, 0);
    for (int r = 0; r < R && !err; ++r) {
        tfidf_run_info ri;
        memset(&ri, 0, sizeof(ri));
        ri.size = sizeof(ri);
        err = tfidf_last_run_info(g->ctx[r], &ri);
        doc0[r + 1] = doc0[r] + ri.ndocs;
        pair0[r + 1] = pair0[r] + ri.npairs;
    }
    /* (rank, row in the rank's part) of every output row; rank -1: no rank holds the id */
    std::vector<int> src_rank;
    std::vector<uint32_t> src_row;
    if (!err) {
        if (!doc_ids) {
            for (int r = 0; r < R; ++r)
                for (uint32_t i = 0; i < part[r].ndocs; ++i) { src_rank.push_back(r); src_row.push_back(i); }
        } else {
            for (uint32_t i = 0; i < ndocs; ++i) {
                int h = -1;
                for (int r = 0; r < R && h < 0; ++r)
                    if (part[r].pos[i] != UINT32_MAX) h = r;
                src_rank.push_back(h);
                src_row.push_back(i);
            }
        }
        if (src_rank.size() > 0xFFFFFFFFull) err = TFIDF_E_CAPACITY;
    }
    tfidf_doc_terms m;
    memset(&m, 0, sizeof(m));
    const size_t nr = src_rank.size(), nrk = nr * k;
    uint64_t wtotal = 0;
    if (!err) {
        for (size_t i = 0; i < nr; ++i)
            if (src_rank[i] >= 0) {
                const tfidf_doc_terms& p = part[src_rank[i]];
                const size_t e = (size_t)src_row[i] * k;
                wtotal += p.word_off[e + k] - p.word_off[e];
            }
        m.ndocs = (uint32_t)nr;
        m.k = k;
        m.doc = (uint32_t*)calloc(nr + 1, 4);
        m.pos = (uint32_t*)calloc(nr + 1, 4);
        m.npairs = (uint64_t*)calloc(nr + 1, 8);
        m.nterms = (uint32_t*)calloc(nr + 1, 4);
        m.term = (uint32_t*)calloc(nrk + 1, 4);
        m.count = (uint32_t*)calloc(nrk + 1, 4);
        m.score = (double*)calloc(nrk + 1, 8);
        m.pair = (uint64_t*)calloc(nrk + 1, 8);
        m.word_off = (uint64_t*)calloc(nrk + 1, 8);
        m.word_bytes = (uint8_t*)calloc((size_t)wtotal + 1, 1);
        if (!m.doc || !m.pos || !m.npairs || !m.nterms || !m.term || !m.count || !m.score || !m.pair || !m.word_off ||
            !m.word_bytes)
            err = TFIDF_E_NOMEM;
    }
    uint64_t wat = 0;
    for (size_t i = 0; i < nr && !err; ++i) {
        const size_t o = i * k;
        const int h = src_rank[i];
        if (h < 0) {
            m.doc[i] = doc_ids[i];
            m.pos[i] = UINT32_MAX;
            for (uint32_t j = 0; j < k; ++j) m.word_off[o + j] = wat;
            continue;
        }
        const tfidf_doc_terms& p = part[h];
        const uint32_t r = src_row[i];
        const size_t e = (size_t)r * k;
        m.doc[i] = p.doc[r];
        m.pos[i] = (uint32_t)(doc0[h] + p.pos[r]);
        m.npairs[i] = p.npairs[r];
        m.nterms[i] = p.nterms[r];
        memcpy(m.term + o, p.term + e, (size_t)k * 4);
        memcpy(m.count + o, p.count + e, (size_t)k * 4);
        memcpy(m.score + o, p.score + e, (size_t)k * 8);
        for (uint32_t j = 0; j < k; ++j) {
            m.pair[o + j] = j < p.nterms[r] ? pair0[h] + p.pair[e + j] : 0;
            m.word_off[o + j] = wat + (p.word_off[e + j] - p.word_off[e]);
        }
        const uint64_t wn = p.word_off[e + k] - p.word_off[e];
        if (wn) memcpy(m.word_bytes + wat, p.word_bytes + p.word_off[e], (size_t)wn);
        wat += wn;
    }
    if (!err) m.word_off[nrk] = wat;
    for (tfidf_doc_terms& p : part) tfidf_doc_terms_free(&p);
    if (err) {
        tfidf_doc_terms_free(&m);
        memset(out, 0, sizeof(*out));
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

/* The rank that holds a row's document exports its vector as (word bytes, score) and its norm
 * (tfidf_ctx_similar_export, every rank on its own host thread); the rows are put together
 * here (NULL list: the ranks' rows in rank order; id list: each row from the first rank that
 * holds the id, an id nobody holds stays empty); every rank then searches its shard for all
 * rows (tfidf_ctx_similar_ext) and the ranks' rows are merged by (sim descending, document id
 * ascending).  The words sort the same in every shard, so a rank adds a row's shared terms in
 * the order a single shard would, and the shards partition the documents: the merged top-k is
 * the single-shard result bit for bit. */
int tfidf_group_similar(tfidf_group* g, const uint32_t* doc_ids, uint32_t ndocs, uint32_t k, tfidf_neighbors* out) {
    if (!g || !out) return TFIDF_E_INVAL;
    if (k == 0 || k > TFIDF_SIMILAR_MAX_K) return TFIDF_E_INVAL;
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<SimExport> ex((size_t)R);
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r) th.emplace_back([&, r] { rc[r] = tfidf_ctx_similar_export(g->ctx[r], doc_ids, ndocs, &ex[r]); });
        rc[0] = tfidf_ctx_similar_export(g->ctx[0], doc_ids, ndocs, &ex[0]);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    std::vector<uint64_t> doc0((size_t)R + 1, 0);
    for (int r = 0; r < R && !err; ++r) {
        tfidf_run_info ri;
        memset(&ri, 0, sizeof(ri));
        ri.size = sizeof(ri);
        err = tfidf_last_run_info(g->ctx[r], &ri);
        doc0[r + 1] = doc0[r] + ri.ndocs;
    }
    /* (rank, row in the rank's export) of every row; rank -1: no rank holds the id */
    std::vector<int> src_rank;
    std::vector<uint32_t> src_row;
    if (!err) {
        if (!doc_ids) {
            for (int r = 0; r < R; ++r)
                for (size_t i = 0; i + 1 < ex[r].voff.size(); ++i) { src_rank.push_back(r); src_row.push_back((uint32_t)i); }
        } else {
            for (uint32_t i = 0; i < ndocs; ++i) {
                int h = -1;
                for (int r = 0; r < R && h < 0; ++r)
                    if (ex[r].pos[i] != UINT32_MAX) h = r;
                src_rank.push_back(h);
                src_row.push_back(i);
            }
        }
        if (src_rank.size() > 0xFFFFFFFFull) err = TFIDF_E_CAPACITY;
    }
    const size_t nr = src_rank.size();
    SimExport all;
    tfidf_neighbors m;
    memset(&m, 0, sizeof(m));
    if (!err) {
        all.id.assign(nr + 1, 0);
        all.norm.assign(nr + 1, 0.0);
        all.voff.assign(nr + 1, 0);
        all.woff.assign(1, 0);
        for (size_t i = 0; i < nr; ++i) {
            const int h = src_rank[i];
            all.id[i] = h < 0 ? doc_ids[i] : ex[h].id[src_row[i]];
            uint64_t np = 0;
            if (h >= 0) {
                const SimExport& e = ex[h];
                const uint32_t x = src_row[i];
                all.norm[i] = e.norm[x];
                np = e.voff[x + 1] - e.voff[x];
                const uint64_t w0 = e.woff[e.voff[x]], wat = all.wbytes.size();
                for (uint64_t p = e.voff[x]; p < e.voff[x + 1]; ++p) {
                    all.score.push_back(e.score[p]);
                    all.woff.push_back(wat + (e.woff[p + 1] - w0));
                }
                all.wbytes.insert(all.wbytes.end(), e.wbytes.begin() + (size_t)w0, e.wbytes.begin() + (size_t)e.woff[e.voff[x + 1]]);
            }
            all.voff[i + 1] = all.voff[i] + np;
        }
    }
    std::vector<tfidf_neighbors> part((size_t)R);
    for (tfidf_neighbors& p : part) memset(&p, 0, sizeof(p));
    if (!err) {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r) th.emplace_back([&, r] { rc[r] = tfidf_ctx_similar_ext(g->ctx[r], &all, k, &part[r]); });
        rc[0] = tfidf_ctx_similar_ext(g->ctx[0], &all, k, &part[0]);
        for (auto& t : th) t.join();
        for (int r = 0; r < R && !err; ++r) err = rc[r];
    }
    if (!err) {
        m.ndocs = (uint32_t)nr;
        m.k = k;
        m.doc = (uint32_t*)calloc(nr + 1, 4);
        m.pos = (uint32_t*)calloc(nr + 1, 4);
        m.npairs = (uint64_t*)calloc(nr + 1, 8);
        m.norm = (double*)calloc(nr + 1, 8);
        m.nmatch = (uint64_t*)calloc(nr + 1, 8);
        m.nnb = (uint32_t*)calloc(nr + 1, 4);
        m.nb_doc = (uint32_t*)calloc(nr * k + 1, 4);
        m.nb_shared = (uint32_t*)calloc(nr * k + 1, 4);
        m.nb_score = (double*)calloc(nr * k + 1, 8);
        if (!m.doc || !m.pos || !m.npairs || !m.norm || !m.nmatch || !m.nnb || !m.nb_doc || !m.nb_shared || !m.nb_score)
            err = TFIDF_E_NOMEM;
    }
    for (size_t i = 0; i < nr && !err; ++i) {
        const int h = src_rank[i];
        m.doc[i] = all.id[i];
        m.pos[i] = h < 0 ? UINT32_MAX : (uint32_t)(doc0[h] + ex[h].pos[src_row[i]]);
        m.npairs[i] = all.voff[i + 1] - all.voff[i];
        m.norm[i] = all.norm[i];
        std::vector<size_t> at((size_t)R, 0);   /* R-way merge of the ranks' ordered rows */
        uint32_t n = 0;
        for (int r = 0; r < R; ++r) m.nmatch[i] += part[r].nmatch[i];
        while (n < k) {
            int best = -1;
            uint64_t bs = 0;
            uint32_t bd = 0;
            for (int r = 0; r < R; ++r) {
                if (at[r] >= part[r].nnb[i]) continue;
                uint64_t sb;
                memcpy(&sb, &part[r].nb_score[i * k + at[r]], 8);   /* sims >= +0.0: the bits order like the values */
                const uint32_t d = part[r].nb_doc[i * k + at[r]];
                if (best < 0 || sb > bs || (sb == bs && d < bd)) { best = r; bs = sb; bd = d; }
            }
            if (best < 0) break;
            m.nb_doc[i * k + n] = bd;
            m.nb_shared[i * k + n] = part[best].nb_shared[i * k + at[best]];
            memcpy(&m.nb_score[i * k + n], &bs, 8);
            ++at[best];
            ++n;
        }
        m.nnb[i] = n;
    }
    for (tfidf_neighbors& p : part) tfidf_neighbors_free(&p);
    if (err) {
        tfidf_neighbors_free(&m);
        memset(out, 0, sizeof(*out));
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

/* strcmp order of "a\t" and "b\t" (TFIDF.c:245,273): words hold no NUL and no whitespace, so
 * the TAB meets a byte it differs from when one word is a prefix of the other */
static int word_tab_cmp(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    const uint32_t n = na < nb ? na : nb;
    const int c = n ? memcmp(a, b, n) : 0;
    if (c || na == nb) return c;
    return na < nb ? (0x09 < b[n] ? -1 : 1) : (a[n] < 0x09 ? -1 : 1);
}

/* Every rank transforms the whole batch against its own vocabulary (tfidf_transform is local
 * to a context), one host thread per rank as in tfidf_group_run.  Term-table order is the
 * word order in every shard, so each rank's row is sorted by word and the rows merge by a
 * k-way merge over the batch's bytes; a pair several ranks hold (equal word_off: the term's
 * first token in the document) is kept once — df and N are global, so the ranks agree on it. */
int tfidf_group_transform(tfidf_group* g, const tfidf_corpus* batch, tfidf_rows* out) {
    if (!g || !batch || !out) return TFIDF_E_INVAL;
    if (batch->flags & TFIDF_CORPUS_DEVICE) return TFIDF_E_INVAL;   /* the merge reads the words on the host */
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_rows> part((size_t)R);
    for (tfidf_rows& p : part) memset(&p, 0, sizeof(p));
    {
        std::vector<std::thread> th;
        /* under a row norm the ranks return w: a rank sees only its own vocabulary's part of a row */
        for (int r = 1; r < R; ++r) th.emplace_back([&, r] { rc[r] = tfidf_ctx_transform(g->ctx[r], batch, &part[r], false); });
        rc[0] = tfidf_ctx_transform(g->ctx[0], batch, &part[0], false);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    const uint32_t N = batch->ndocs;
    tfidf_weighting wt;
    memset(&wt, 0, sizeof(wt));
    wt.size = sizeof(wt);
    if (!err) err = tfidf_weighting_get(g->ctx[0], &wt);   /* the same on every rank (tfidf_group_reweight) */
    tfidf_rows m;
    memset(&m, 0, sizeof(m));
    uint64_t cap = 0;
    for (int r = 0; r < R && !err; ++r) cap += part[r].npairs;
    if (!err) {
        m.ndocs = N;
        m.ntokens = part[0].ntokens;
        m.row_off = (uint64_t*)calloc((size_t)N + 1, 8);
        m.doc_size = (uint32_t*)calloc((size_t)N + 1, 4);
        m.doc_oov = (uint32_t*)calloc((size_t)N + 1, 4);
        m.term = (uint32_t*)calloc((size_t)cap + 1, 4);
        m.count = (uint32_t*)calloc((size_t)cap + 1, 4);
        m.df = (uint32_t*)calloc((size_t)cap + 1, 4);
        m.score = (double*)calloc((size_t)cap + 1, 8);
        m.word_off = (uint64_t*)calloc((size_t)cap + 1, 8);
        m.word_len = (uint32_t*)calloc((size_t)cap + 1, 4);
        if (!m.row_off || !m.doc_size || !m.doc_oov || !m.term || !m.count || !m.df || !m.score || !m.word_off || !m.word_len)
            err = TFIDF_E_NOMEM;
    }
    uint64_t P = 0;
    std::vector<uint64_t> at((size_t)R);
    for (uint32_t d = 0; d < N && !err; ++d) {
        m.row_off[d] = P;
        m.doc_size[d] = part[0].doc_size[d];
        uint64_t in_vocab = 0;
        for (int r = 0; r < R; ++r) at[r] = part[r].row_off[d];
        for (;;) {
            int best = -1;
            for (int r = 0; r < R; ++r) {
                if (at[r] >= part[r].row_off[d + 1]) continue;
                if (best < 0 || word_tab_cmp(batch->bytes + part[r].word_off[at[r]], part[r].word_len[at[r]],
                                             batch->bytes + part[best].word_off[at[best]], part[best].word_len[at[best]]) < 0)
                    best = r;
            }
            if (best < 0) break;
            const uint64_t x = at[best], wo = part[best].word_off[x];
            m.term[P] = 0xFFFFFFFFu;
            m.count[P] = part[best].count[x];
            m.df[P] = part[best].df[x];
            m.score[P] = part[best].score[x];
            m.word_off[P] = wo;
            m.word_len[P] = part[best].word_len[x];
            in_vocab += m.count[P];
            ++P;
            for (int r = 0; r < R; ++r)   /* the same pair on the other ranks */
                if (at[r] < part[r].row_off[d + 1] && part[r].word_off[at[r]] == wo) ++at[r];
        }
        m.doc_oov[d] = (uint32_t)(m.doc_size[d] - in_vocab);
        /* the merged row is in pair order: the scheme's norm by the host definition (weight_host.c) */
        if (wt.norm != TFIDF_NORM_NONE) (void)tfidf_weight_normalize(m.score + m.row_off[d], P - m.row_off[d], wt.norm);
    }
    if (!err) {
        m.row_off[N] = P;
        m.npairs = P;
    }
    for (tfidf_rows& p : part) tfidf_rows_free(&p);
    if (err) {
        tfidf_rows_free(&m);
        memset(out, 0, sizeof(*out));
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

/* Every rank exports its own term table (tfidf_model_export is local to a context), one host
 * thread per rank; each table is in strcmp("word\t") order, so the group's table is their
 * k-way merge in that order.  A word several ranks hold is kept once: df is global, so the
 * ranks agree on it (a disagreement is reported, not resolved).  N is the run's on every rank. */
int tfidf_group_model_export(tfidf_group* g, tfidf_model* out) {
    if (!g || !out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_model> part((size_t)R);
    for (tfidf_model& p : part) memset(&p, 0, sizeof(p));
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r) th.emplace_back([&, r] { rc[r] = tfidf_model_export(g->ctx[r], &part[r]); });
        rc[0] = tfidf_model_export(g->ctx[0], &part[0]);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    for (int r = 1; r < R && !err; ++r)
        if (part[r].ndocs_total != part[0].ndocs_total) err = TFIDF_E_STATE;
    tfidf_model m;
    memset(&m, 0, sizeof(m));
    uint64_t vsum = 0, bsum = 0;
    for (int r = 0; r < R && !err; ++r) {
        vsum += part[r].nterms;
        bsum += part[r].term_off[part[r].nterms];
    }
    if (!err) {
        m.size = sizeof(tfidf_model);
        m.ndocs_total = part[0].ndocs_total;
        m.term_off = (uint64_t*)calloc((size_t)vsum + 1, 8);
        m.term_df = (uint32_t*)calloc((size_t)vsum + 1, 4);
        m.term_bytes = (uint8_t*)malloc((size_t)bsum + 1);
        if (!m.term_off || !m.term_df || !m.term_bytes) err = TFIDF_E_NOMEM;
    }
    uint64_t V = 0, B = 0;
    std::vector<uint32_t> at((size_t)R, 0u);
    while (!err) {
        int best = -1;
        for (int r = 0; r < R; ++r) {
            if (at[r] >= part[r].nterms) continue;
            const tfidf_model& p = part[r];
            if (best < 0) { best = r; continue; }
            const tfidf_model& q = part[best];
            if (word_tab_cmp(p.term_bytes + p.term_off[at[r]], (uint32_t)(p.term_off[at[r] + 1] - p.term_off[at[r]]),
                             q.term_bytes + q.term_off[at[best]],
                             (uint32_t)(q.term_off[at[best] + 1] - q.term_off[at[best]])) < 0)
                best = r;
        }
        if (best < 0) break;
        const tfidf_model& q = part[best];
        const uint64_t wo = q.term_off[at[best]], wl = q.term_off[at[best] + 1] - wo;
        const uint32_t df = q.term_df[at[best]];
        if (V >= 0xFFFFFFFEull) { err = TFIDF_E_CAPACITY; break; }
        m.term_off[V] = B;
        memcpy(m.term_bytes + B, q.term_bytes + wo, (size_t)wl);
        m.term_df[V] = df;
        for (int r = 0; r < R; ++r) {   /* the same word on the other ranks (and this one) */
            if (at[r] >= part[r].nterms) continue;
            const tfidf_model& p = part[r];
            const uint64_t po = p.term_off[at[r]], pl = p.term_off[at[r] + 1] - po;
            if (pl != wl || (wl && memcmp(p.term_bytes + po, m.term_bytes + B, (size_t)wl) != 0)) continue;
            if (p.term_df[at[r]] != df) err = TFIDF_E_STATE;
            ++at[r];
        }
        B += wl;
        ++V;
    }
    if (!err) {
        m.term_off[V] = B;
        m.nterms = (uint32_t)V;
    }
    for (tfidf_model& p : part) tfidf_model_free(&p);
    if (err) {
        tfidf_model_free(&m);
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

/* Every rank matches the patterns against its own term table (tfidf_match_terms is local to a
 * context), one host thread per rank.  A row is ordered by (dist, df descending, "word\t"), and a
 * word has the same dist and the same global df in every shard that holds it, so the ranks' rows
 * merge by that key and a word several ranks return is kept once: the first E of the merge are
 * the first E of the corpus-wide dictionary.  nmatch is the largest rank's count. */
int tfidf_group_match_terms(tfidf_group* g, const tfidf_patterns* patterns, const tfidf_match_params* params,
                            tfidf_term_matches* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!g || tfidf_match_check(patterns, params) != TFIDF_OK) return TFIDF_E_INVAL;
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_term_matches> part((size_t)R);
    for (tfidf_term_matches& p : part) memset(&p, 0, sizeof(p));
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r)
            th.emplace_back([&, r] { rc[r] = tfidf_match_terms(g->ctx[r], patterns, params, &part[r]); });
        rc[0] = tfidf_match_terms(g->ctx[0], patterns, params, &part[0]);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    const uint32_t P = patterns->npatterns, E = params->max_expansions;
    const size_t PE = (size_t)P * E;
    tfidf_term_matches m;
    memset(&m, 0, sizeof(m));
    uint64_t bsum = 0;
    for (int r = 0; r < R && !err; ++r) bsum += part[r].word_off[PE];
    if (!err) {
        m.npatterns = P;
        m.k = E;
        m.nmatch = (uint64_t*)calloc((size_t)P + 1, 8);
        m.nterms = (uint32_t*)calloc((size_t)P + 1, 4);
        m.term = (uint32_t*)calloc(PE + 1, 4);
        m.dist = (uint8_t*)calloc(PE + 1, 1);
        m.df = (uint32_t*)calloc(PE + 1, 4);
        m.word_off = (uint64_t*)calloc(PE + 1, 8);
        m.word_bytes = (uint8_t*)malloc((size_t)bsum + 1);
        if (!m.nmatch || !m.nterms || !m.term || !m.dist || !m.df || !m.word_off || !m.word_bytes) err = TFIDF_E_NOMEM;
    }
    uint64_t B = 0;
    std::vector<uint32_t> at((size_t)R);
    for (uint32_t p = 0; p < P && !err; ++p) {
        for (int r = 0; r < R; ++r) {
            at[r] = 0;
            if (part[r].nmatch[p] > m.nmatch[p]) m.nmatch[p] = part[r].nmatch[p];
        }
        uint32_t n = 0;
        for (; n < E; ++n) {
            int best = -1;
            size_t be = 0;
            for (int r = 0; r < R; ++r) {
                if (at[r] >= part[r].nterms[p]) continue;
                const tfidf_term_matches& q = part[r];
                const size_t e = (size_t)p * E + at[r];
                bool first = best < 0;
                if (!first) {
                    const tfidf_term_matches& b = part[best];
                    if (q.dist[e] != b.dist[be]) first = q.dist[e] < b.dist[be];
                    else if (q.df[e] != b.df[be]) first = q.df[e] > b.df[be];
                    else first = word_tab_cmp(q.word_bytes + q.word_off[e], (uint32_t)(q.word_off[e + 1] - q.word_off[e]),
                                              b.word_bytes + b.word_off[be], (uint32_t)(b.word_off[be + 1] - b.word_off[be])) < 0;
                }
                if (first) { best = r; be = e; }
            }
            if (best < 0) break;
            const tfidf_term_matches& b = part[best];
            const uint64_t wl = b.word_off[be + 1] - b.word_off[be];
            const size_t o = (size_t)p * E + n;
            m.term[o] = 0xFFFFFFFFu;
            m.dist[o] = b.dist[be];
            m.df[o] = b.df[be];
            m.word_off[o] = B;
            memcpy(m.word_bytes + B, b.word_bytes + b.word_off[be], (size_t)wl);
            for (int r = 0; r < R; ++r) {   /* the same word on the other ranks (and this one) */
                if (at[r] >= part[r].nterms[p]) continue;
                const tfidf_term_matches& q = part[r];
                const size_t e = (size_t)p * E + at[r];
                const uint64_t ql = q.word_off[e + 1] - q.word_off[e];
                if (ql == wl && (!wl || memcmp(q.word_bytes + q.word_off[e], m.word_bytes + B, (size_t)wl) == 0)) ++at[r];
            }
            B += wl;
        }
        m.nterms[p] = n;
        for (uint32_t j = n; j < E; ++j) m.word_off[(size_t)p * E + j] = B;
    }
    if (!err) m.word_off[PE] = B;
    for (tfidf_term_matches& p : part) tfidf_term_matches_free(&p);
    if (err) {
        tfidf_term_matches_free(&m);
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

/* Every rank gets the whole job list on its own host thread and answers TFIDF_SNIP_NO_DOC for what it
 * does not hold; each job is taken from the first rank that held it.  Slots index U(q), which every
 * rank derives from the same query bytes, so a job's fields are a single shard's; a term counts as
 * found when any rank found it. */
int tfidf_group_snippet(tfidf_group* g, const tfidf_queries* queries, const uint32_t* job_query, const uint32_t* job_doc,
                        uint32_t njobs, const tfidf_snippet_params* params, tfidf_snippets* out) {
    if (!out) return TFIDF_E_INVAL;
    memset(out, 0, sizeof(*out));
    if (!g) return TFIDF_E_INVAL;
    const int R = g->n;
    std::vector<int> rc((size_t)R, TFIDF_OK);
    std::vector<tfidf_snippets> part((size_t)R);
    for (tfidf_snippets& p : part) memset(&p, 0, sizeof(p));
    {
        std::vector<std::thread> th;
        for (int r = 1; r < R; ++r)
            th.emplace_back([&, r] { rc[r] = tfidf_snippet(g->ctx[r], queries, job_query, job_doc, njobs, params, &part[r]); });
        rc[0] = tfidf_snippet(g->ctx[0], queries, job_query, job_doc, njobs, params, &part[0]);
        for (auto& t : th) t.join();
    }
    int err = TFIDF_OK;
    for (int r = 0; r < R && !err; ++r) err = rc[r];
    tfidf_snippets m;
    memset(&m, 0, sizeof(m));
    std::vector<int> from((size_t)njobs, 0);
    uint64_t nmarks = 0, ntext = 0, nT = 0;
    if (!err) {
        for (uint32_t j = 0; j < njobs; ++j) {
            int r = 0;
            while (r < R && (part[r].flags[j] & TFIDF_SNIP_NO_DOC)) ++r;
            from[j] = r < R ? r : 0;
            const tfidf_snippets& p = part[from[j]];
            nmarks += p.mark_off[j + 1] - p.mark_off[j];
            ntext += p.text_off[j + 1] - p.text_off[j];
        }
        const uint32_t nq = part[0].nqueries;
        nT = part[0].qterm_off[nq];
        m.njobs = njobs;
        m.nqueries = nq;
        m.flags = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.ntokens = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.nmatch = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.nterms_matched = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.win_tok = (uint32_t*)calloc(2 * (size_t)njobs + 1, 4);
        m.win_byte = (uint64_t*)calloc(2 * (size_t)njobs + 1, 8);
        m.cover = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.hits = (uint32_t*)calloc((size_t)njobs + 1, 4);
        m.mark_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
        m.text_off = (uint64_t*)calloc((size_t)njobs + 1, 8);
        m.mark_byte = (uint64_t*)calloc((size_t)nmarks + 1, 8);
        m.mark_len = (uint32_t*)calloc((size_t)nmarks + 1, 4);
        m.mark_slot = (uint32_t*)calloc((size_t)nmarks + 1, 4);
        m.text = (uint8_t*)calloc((size_t)ntext + 1, 1);
        m.qterm_off = (uint64_t*)calloc((size_t)nq + 1, 8);
        m.qterm_pos = (uint64_t*)calloc((size_t)nT + 1, 8);
        m.qterm_len = (uint32_t*)calloc((size_t)nT + 1, 4);
        m.qterm_found = (uint8_t*)calloc((size_t)nT + 1, 1);
        if (!m.flags || !m.ntokens || !m.nmatch || !m.nterms_matched || !m.win_tok || !m.win_byte || !m.cover || !m.hits ||
            !m.mark_off || !m.text_off || !m.mark_byte || !m.mark_len || !m.mark_slot || !m.text || !m.qterm_off ||
            !m.qterm_pos || !m.qterm_len || !m.qterm_found)
            err = TFIDF_E_NOMEM;
    }
    if (!err) {
        uint64_t M = 0, B = 0;
        for (uint32_t j = 0; j < njobs; ++j) {
            const tfidf_snippets& p = part[from[j]];
            m.flags[j] = p.flags[j];
            m.ntokens[j] = p.ntokens[j];
            m.nmatch[j] = p.nmatch[j];
            m.nterms_matched[j] = p.nterms_matched[j];
            m.win_tok[2 * (size_t)j] = p.win_tok[2 * (size_t)j];
            m.win_tok[2 * (size_t)j + 1] = p.win_tok[2 * (size_t)j + 1];
            m.win_byte[2 * (size_t)j] = p.win_byte[2 * (size_t)j];
            m.win_byte[2 * (size_t)j + 1] = p.win_byte[2 * (size_t)j + 1];
            m.cover[j] = p.cover[j];
            m.hits[j] = p.hits[j];
            m.mark_off[j] = M;
            m.text_off[j] = B;
            const uint64_t nm = p.mark_off[j + 1] - p.mark_off[j], nb = p.text_off[j + 1] - p.text_off[j];
            if (nm) {
                memcpy(m.mark_byte + M, p.mark_byte + p.mark_off[j], (size_t)nm * 8);
                memcpy(m.mark_len + M, p.mark_len + p.mark_off[j], (size_t)nm * 4);
                memcpy(m.mark_slot + M, p.mark_slot + p.mark_off[j], (size_t)nm * 4);
            }
            if (nb) memcpy(m.text + B, p.text + p.text_off[j], (size_t)nb);
            M += nm;
            B += nb;
        }
        m.mark_off[njobs] = M;
        m.text_off[njobs] = B;
        memcpy(m.qterm_off, part[0].qterm_off, ((size_t)m.nqueries + 1) * 8);
        if (nT) {
            memcpy(m.qterm_pos, part[0].qterm_pos, (size_t)nT * 8);
            memcpy(m.qterm_len, part[0].qterm_len, (size_t)nT * 4);
        }
        for (int r = 0; r < R; ++r)
            for (uint64_t x = 0; x < nT; ++x) m.qterm_found[x] |= part[r].qterm_found[x];
    }
    for (tfidf_snippets& p : part) tfidf_snippets_free(&p);
    if (err) {
        tfidf_snippets_free(&m);
        return err;
    }
    *out = m;
    return TFIDF_OK;
}

void tfidf_group_close(tfidf_group* g) {
    if (!g) return;
    for (tfidf_ctx* c : g->ctx)
        if (c) tfidf_close(c);
    delete g->hub;
    delete g;
}

}  // extern "C"
