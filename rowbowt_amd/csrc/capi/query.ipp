// capi/query.ipp -- what the query entry points share: queryable(), the staging of a host read batch (ReadBatch), check_offsets(), make_order(), host memory for
// results (the result pool behind alloc_result; rbg_free_buffer, load.ipp, gives blocks back) and the big copies through pinned staging (d2h_result, h2d_big), ragged_finish().  Part of rbg_capi.hip.
namespace {
bool queryable(const rbg_index *ix) { return ix && ix->device != RBG_DEVICE_NONE; }

// common staging for host read batches
struct ReadBatch {
    DevBuf seqs, off;
    int stage(const uint8_t *h_seqs, const uint64_t *h_off, uint64_t N, hipStream_t st) {
        const uint64_t total = N ? h_off[N] : 0;
        int rc;
        if ((rc = seqs.alloc(((total + 15) & ~uint64_t(15)) + 16))) return rc;
        if ((rc = off.alloc((N + 1) * 8))) return rc;
        if (total) HIP_TRY(hipMemcpyAsync(seqs.p, h_seqs, total, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(off.p, h_off, (N + 1) * 8, hipMemcpyHostToDevice, st));
        return RBG_OK;
    }
};

// host-pointer locate paths: order the chains when the batch is big enough for the sort to pay
int make_order(rbg_index *ix, const uint64_t *d_k, uint64_t N, DevBuf &ws, hipStream_t st, const void **order) {
    *order = nullptr;
    if (N < 4096 || N >= 0xFFFFFFFFull) return RBG_OK;
    const size_t bytes = locate_order_ws_bytes(N);
    int rc = ws.alloc(bytes);
    if (rc) return rc;
    if (launch_locate_order(ix->dev, ix->cfg, d_k, N, ws.p, bytes, st)) return RBG_ENODEV;
    *order = ws.p;
    return RBG_OK;
}

int check_offsets(const uint64_t *off, uint64_t N) {
    if (N == 0) return RBG_OK;
    if (!off || off[0] != 0) return RBG_EARG;
    for (uint64_t i = 0; i < N; ++i)
        if (off[i + 1] < off[i]) return RBG_EARG;
    return RBG_OK;
}

// Host memory for a ragged result (released by rbg_free_buffer = free).  The device-to-host copy is the
// first touch of this memory, and for gigabytes of locations the page faults cost more than the PCIe
// transfer (tools/d2h_probe.hip: 3 GB in 0.22 s into fresh malloc memory, 0.13-0.16 s into 2 MB-aligned
// memory marked for transparent huge pages, 0.06 s once touched), so large results ask for huge pages.
// Large results are RECYCLED: rbg_free_buffer keeps blocks of 8 MB and more (up to 6 GB in all) and the next result
// of about that size gets one whose pages are already there -- a batch loop (rb_markers: 1 GB of seed records per 2 M reads;
// rbg_locs_at: 3 GB per 10 M reads) otherwise faults the same pages in again at every call, which costs more than the copy
// (0.098 s of copy-out per 2 M reads in rb_markers, 0.03 s with recycled blocks).  RBG_RESULT_POOL=0 switches it off.
struct ResultPool {
    std::mutex mu;
    std::map<void *, size_t> live;            // blocks handed out by alloc_result (pooled sizes only)
    std::multimap<size_t, void *> idle;
    size_t cached = 0;
    const bool on = !(std::getenv("RBG_RESULT_POOL") && std::getenv("RBG_RESULT_POOL")[0] == '0');
    static constexpr size_t kMax = size_t(6) << 30;
    static ResultPool &get() { static ResultPool p; return p; }
    ~ResultPool() { for (auto &kv : idle) std::free(kv.second); }
};
void *alloc_result(size_t bytes) {
    constexpr size_t kHuge = size_t(2) << 20;
    ResultPool &P = ResultPool::get();
    if (bytes >= 4 * kHuge) {
        const size_t rounded = (bytes + kHuge - 1) & ~(kHuge - 1);
        if (P.on) {
            std::lock_guard<std::mutex> g(P.mu);
            auto it = P.idle.lower_bound(rounded);
            if (it != P.idle.end() && it->first <= rounded + rounded / 4) {
                void *p = it->second;
                P.live[p] = it->first;
                P.cached -= it->first;
                P.idle.erase(it);
                return p;
            }
        }
        void *p = std::aligned_alloc(kHuge, rounded);
        if (p) {
            (void)madvise(p, rounded, MADV_HUGEPAGE);
            if (P.on) { std::lock_guard<std::mutex> g(P.mu); P.live[p] = rounded; }
            return p;
        }
    }
    return std::malloc(bytes ? bytes : 8);
}

// pinned staging of big ragged results (ragged_finish): four 64 MB buffers per process, allocated on first use
struct PinnedStage {
    static constexpr size_t kChunk = size_t(64) << 20;
    static constexpr int kBufs = 4;
    std::mutex mu;
    void *buf[kBufs] = {nullptr, nullptr, nullptr, nullptr};   // portable: any device of the process may copy into them
    bool ok = false, tried = false;
    static PinnedStage &get() { static PinnedStage p; return p; }
    bool ensure() {   // (under mu)
        if (tried) return ok;
        tried = true;
        for (int i = 0; i < kBufs; ++i)
            if (rbg_numa::host_malloc_near(&buf[i], kChunk, hipHostMallocPortable, [] { int d = 0; (void)hipGetDevice(&d); return d; }()) != hipSuccess) {
                (void)hipGetLastError();
                return ok = false;
            }
        return ok = true;
    }
};

// Device-to-host copy of a (possibly huge) result into memory that may never have been touched.  Big results leave
// through pinned staging: a copy straight into fresh pageable memory is the first touch of its pages, and for gigabytes
// of locations the page faults (and the driver's own staging) cost more than the transfer (tools/d2h_probe.hip: 3 GB in
// 0.2 s; 0.06 s for the DMA alone).  Chunks of 64 MB are copied into four pinned buffers, two copies ahead, and a team
// of worker threads moves each finished chunk to its place -- which is where the pages get touched, by sixteen threads
// at once and alongside the next chunks' DMA.  Blocks until the data has arrived.
int d2h_result(void *h_dst, const void *d_src, size_t bytes, hipStream_t st) {
    if (bytes == 0) return RBG_OK;
    if (bytes >= (size_t(64) << 20)) {
        PinnedStage &ps = PinnedStage::get();
        std::unique_lock<std::mutex> lk(ps.mu, std::try_to_lock);   // (one big result at a time goes this way; a second caller takes the plain copy)
        if (lk.owns_lock() && ps.ensure()) {
            const size_t chunk = PinnedStage::kChunk;
            const size_t nb = (bytes + chunk - 1) / chunk;
            const unsigned T = std::max(1u, std::min(16u, rbg_hostpath::cpu_budget()));
            rbg_hostpath::ThreadTeam team(T);
            char *dst = static_cast<char *>(h_dst);
            const char *src = static_cast<const char *>(d_src);
            hipError_t e = hipSuccess;
            hipEvent_t ev[PinnedStage::kBufs] = {nullptr, nullptr, nullptr, nullptr};   // (per call: events belong to the current device)
            for (hipEvent_t &x : ev)
                if (e == hipSuccess) e = hipEventCreateWithFlags(&x, hipEventDisableTiming);
            auto enqueue = [&](size_t c) {
                const size_t len = std::min(chunk, bytes - c * chunk);
                if (e == hipSuccess) e = hipMemcpyAsync(ps.buf[c % PinnedStage::kBufs], src + c * chunk, len, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipEventRecord(ev[c % PinnedStage::kBufs], st);
            };
            for (size_t c = 0; c < std::min<size_t>(2, nb); ++c) enqueue(c);
            for (size_t c = 0; c < nb && e == hipSuccess; ++c) {
                e = hipEventSynchronize(ev[c % PinnedStage::kBufs]);
                if (e != hipSuccess) break;
                if (c + 2 < nb) enqueue(c + 2);   // its buffer held chunk c - 2, which has been moved out
                const size_t len = std::min(chunk, bytes - c * chunk);
                const char *from = static_cast<const char *>(ps.buf[c % PinnedStage::kBufs]);
                char *to = dst + c * chunk;
                const std::function<void(unsigned)> mv = [&](unsigned t) {
                    const size_t a0 = (len * t / T) & ~size_t(63), z0 = t + 1 == T ? len : (len * (t + 1) / T) & ~size_t(63);
                    if (z0 > a0) std::memcpy(to + a0, from + a0, z0 - a0);
                };
                team.run(mv);
            }
            int rc = RBG_OK;
            if (e != hipSuccess) { (void)hipStreamSynchronize(st); (void)hipGetLastError(); rc = RBG_ENODEV; }
            for (hipEvent_t x : ev)
                if (x) (void)hipEventDestroy(x);
            return rc;
        }
    }
    hipError_t e = hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? RBG_OK : RBG_ENODEV;
}

// The way in for the big arrays of a load (run lists, samples, phi entries: 5-7 GB each at r = 3e8): worker threads
// copy 64 MB chunks of the pageable source into the pinned buffers while the DMA of the chunks before runs -- the
// driver's own path for pageable memory stages through one thread.  RBG_H2D_STAGED=0: plain hipMemcpy (A/B).
int h2d_big(void *d_dst, const void *h_src, size_t bytes) {
    if (bytes == 0) return RBG_OK;
    static const bool staged = [] { const char *e = std::getenv("RBG_H2D_STAGED"); return !(e && e[0] == '0'); }();
    if (staged && bytes >= (size_t(64) << 20)) {
        PinnedStage &ps = PinnedStage::get();
        std::unique_lock<std::mutex> lk(ps.mu, std::try_to_lock);
        if (lk.owns_lock() && ps.ensure()) {
            const size_t chunk = PinnedStage::kChunk;
            const size_t nb = (bytes + chunk - 1) / chunk;
            const unsigned T = std::max(1u, std::min(16u, rbg_hostpath::cpu_budget()));
            rbg_hostpath::ThreadTeam team(T);
            hipStream_t st = hipStreamPerThread;
            char *dst = static_cast<char *>(d_dst);
            const char *src = static_cast<const char *>(h_src);
            hipError_t e = hipSuccess;
            hipEvent_t ev[PinnedStage::kBufs] = {nullptr, nullptr, nullptr, nullptr};
            for (hipEvent_t &x : ev)
                if (e == hipSuccess) e = hipEventCreateWithFlags(&x, hipEventDisableTiming);
            for (size_t c = 0; c < nb && e == hipSuccess; ++c) {
                const int b = static_cast<int>(c % PinnedStage::kBufs);
                if (c >= static_cast<size_t>(PinnedStage::kBufs)) e = hipEventSynchronize(ev[b]);   // chunk c - kBufs has left this buffer
                if (e != hipSuccess) break;
                const size_t len = std::min(chunk, bytes - c * chunk);
                char *to = static_cast<char *>(ps.buf[b]);
                const char *from = src + c * chunk;
                const std::function<void(unsigned)> mv = [&](unsigned t) {
                    const size_t a0 = (len * t / T) & ~size_t(63), z0 = t + 1 == T ? len : (len * (t + 1) / T) & ~size_t(63);
                    if (z0 > a0) std::memcpy(to + a0, from + a0, z0 - a0);
                };
                team.run(mv);
                e = hipMemcpyAsync(dst + c * chunk, ps.buf[b], len, hipMemcpyHostToDevice, st);
                if (e == hipSuccess) e = hipEventRecord(ev[b], st);
            }
            const hipError_t e2 = hipStreamSynchronize(st);
            if (e == hipSuccess) e = e2;
            for (hipEvent_t x : ev)
                if (x) (void)hipEventDestroy(x);
            if (e != hipSuccess) { (void)hipGetLastError(); return RBG_ENODEV; }
            return RBG_OK;
        }
    }
    if (hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return RBG_ENODEV; }
    return RBG_OK;
}

// shared tail of the ragged-output host calls: d_off[N+1] is planned on the device; size, fill, copy back
template <typename FillFn>
int ragged_finish(uint64_t N, DevBuf &d_off, uint64_t *h_off, uint64_t **h_vals, hipStream_t st, FillFn fill) {
    HIP_TRY(hipMemcpyAsync(h_off, d_off.p, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = h_off[N];
    *h_vals = static_cast<uint64_t *>(alloc_result(total * 8));
    if (!*h_vals) return RBG_ENOMEM;
    if (total == 0) return RBG_OK;
    DevBuf d_vals;
    int rc = d_vals.alloc(total * 8);
    if (!rc) rc = fill(d_vals.as<uint64_t>());
    if (!rc) rc = d2h_result(*h_vals, d_vals.p, total * 8, st);
    if (rc) { rbg_free_buffer(*h_vals); *h_vals = nullptr; }
    return rc;
}
}  // namespace
