// capi/tally.ipp -- the marker tally (k_tally.hip): the handle, its reserve rule, add (line mode and per-read mode) / merge / export.  Part of rbg_capi.hip;
// rbg_markers_tally[_reads], the calls that feed a tally from raw reads, are report_pass's third output and sit beside the other two in capi/report.ipp.
//
// THE RESERVE RULE.  The kernels never meet a full table because nothing is launched without room: the host keeps `bound`, an upper bound of the
// claimed slots (the exact count at the last read plus every element handed to a launch since), and a launch of M elements needs
// bound + M <= capacity / 2.  tally_reserve() makes that room: only when the bound says it is missing does it wait for the device, read the exact count
// (8 bytes) and, if the room is still missing, grow -- a new table of at least twice the slots, k_tally_rehash, the old one freed.
struct rbg_tally {
    rbg_index *ix = nullptr;
    uint64_t *slots = nullptr, *hdr = nullptr;   // cap slots of 32 bytes; the header of eight u64 (k_tally.hip)
    uint64_t cap = 0, bound = 0, grows = 0;
    void *ws = nullptr;                          // the element -> record map of an add (launch_report_map's workspace), kept from call to call
    size_t ws_bytes = 0;
    uint64_t *xhdr = nullptr;                    // per-read mode's counters (k_tally_add_reads: four u64), allocated by the first per-read add that has
                                                 // records: a tally that never sees one keeps its create-time allocations
    uint64_t reads = 0;                          // reads seen by per-read adds (counted here: reads without printed records launch nothing)
};

namespace {

int tally_dev_alloc(rbg_index *ix, size_t bytes, void **out) {
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes));
    std::lock_guard<std::mutex> g(ix->mu);
    ix->allocs.push_back({p, bytes});
    ix->hbm_bytes += bytes;
    *out = p;
    return RBG_OK;
}
void tally_dev_free(rbg_index *ix, void *p) {
    std::lock_guard<std::mutex> g(ix->mu);
    free_tracked(ix, p);
}

inline uint64_t tally_room(const rbg_tally *t) { return t->cap / 2 > t->bound ? t->cap / 2 - t->bound : 0; }

// room for `extra` more elements (see above); device work on hipStreamPerThread
int tally_reserve(rbg_tally *t, uint64_t extra) {
    if (extra >> 58) return RBG_EARG;
    if (extra <= tally_room(t)) return RBG_OK;
    HIP_TRY(hipDeviceSynchronize());   // (adds may be in flight on any stream of the caller's)
    uint64_t claimed = 0;
    HIP_TRY(hipMemcpy(&claimed, t->hdr + 5, 8, hipMemcpyDeviceToHost));
    t->bound = claimed;
    if (extra <= tally_room(t)) return RBG_OK;
    uint64_t cap = t->cap * 2;
    while (cap / 2 < claimed + extra) cap <<= 1;
    void *p = nullptr;
    int rc = tally_dev_alloc(t->ix, cap * 32, &p);
    if (rc) return rc;
    hipStream_t st = hipStreamPerThread;
    hipError_t e = static_cast<hipError_t>(launch_tally_clear(static_cast<uint64_t *>(p), cap, st));
    if (e == hipSuccess) e = hipMemsetAsync(t->hdr + 5, 0, 8, st);   // (the re-insertion counts the claimed slots anew)
    if (e == hipSuccess) e = static_cast<hipError_t>(launch_tally_rehash(t->slots, t->cap, static_cast<uint64_t *>(p), cap, t->hdr, st));
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { tally_dev_free(t->ix, p); (void)hipGetLastError(); return RBG_ENODEV; }
    tally_dev_free(t->ix, t->slots);
    t->slots = static_cast<uint64_t *>(p);
    t->cap = cap;
    t->grows += 1;
    return RBG_OK;
}

constexpr uint32_t kTallyFlags = RBG_TALLY_PER_READ | RBG_TALLY_DROP_SITE_CONFLICTS;
inline bool tally_flags_ok(uint32_t f) { return !(f & ~kTallyFlags) && (!(f & RBG_TALLY_DROP_SITE_CONFLICTS) || (f & RBG_TALLY_PER_READ)); }
inline size_t tally_span_bytes(uint64_t R) { return (R * 8 + 255) & ~size_t(255); }

// the add behind launch_report_melem: the map over E = R + M_upper elements (M_upper >= melem[R]), then one lane per element.  The caller has checked
// the room.  Asynchronous on st unless the map's workspace has to grow.  flags (checked by the caller): 0 is line mode; per-read mode also takes the
// records' per-read offsets d_rep_off[N + 1], N >= 1, and d_span, tally_span_bytes(R) of scratch.
int tally_add_mapped(rbg_tally *t, const void *d_recs, uint64_t R, const uint64_t *d_mk, const uint64_t *d_melem, uint64_t M_upper, hipStream_t st,
                     uint32_t flags = 0, const uint64_t *d_rep_off = nullptr, uint64_t N = 0, void *d_span = nullptr) {
    const uint64_t E = R + M_upper;
    const size_t need = report_text_ws_bytes(E);
    if (t->ws_bytes < need) {
        if (t->ws) { HIP_TRY(hipDeviceSynchronize()); tally_dev_free(t->ix, t->ws); t->ws = nullptr; t->ws_bytes = 0; }
        const size_t bytes = need + need / 4;
        int rc = tally_dev_alloc(t->ix, bytes, &t->ws);
        if (rc) return rc;
        t->ws_bytes = bytes;
    }
    if ((flags & RBG_TALLY_PER_READ) && !t->xhdr) {
        void *x = nullptr;
        int rc = tally_dev_alloc(t->ix, 32, &x);
        if (rc) return rc;
        t->xhdr = static_cast<uint64_t *>(x);
        HIP_TRY(hipMemsetAsync(t->xhdr, 0, 32, st));
        HIP_TRY(hipStreamSynchronize(st));   // (once per tally: a later add may come on another stream)
    }
    if (launch_report_map(d_melem, R, E, t->ws, t->ws_bytes, st)) return RBG_ENODEV;
    if (flags & RBG_TALLY_PER_READ) {
        if (launch_tally_add_reads(t->slots, t->cap, t->hdr, t->xhdr, d_recs, d_melem, d_mk, report_map_erec(t->ws), d_rep_off, N, d_span, R, E, flags,
                                   tally_combine_default(), st))
            return RBG_ENODEV;
        t->reads += N;
    } else if (launch_tally_add(t->slots, t->cap, t->hdr, d_recs, d_melem, d_mk, report_map_erec(t->ws), R, E, tally_combine_default(), st)) return RBG_ENODEV;
    t->bound += M_upper;
    return RBG_OK;
}

inline size_t tally_melem_bytes(uint64_t R) { return ((R + 1) * 8 + 255) & ~size_t(255); }
inline uint64_t tally_rotl4(uint64_t m) { return (m << 4) | (m >> 60); }

}  // namespace

extern "C" {

int rbg_tally_create(rbg_index *ix, uint64_t distinct_hint, rbg_tally **out) {
    return guarded([&]() -> int {
    if (!out) return RBG_EARG;
    *out = nullptr;
    if (!queryable(ix)) return RBG_ENODEV;
    if (distinct_hint >> 56) return RBG_EARG;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    std::unique_ptr<rbg_tally> t(new rbg_tally);
    t->ix = ix;
    t->cap = 64;
    while (t->cap < 2 * distinct_hint) t->cap <<= 1;
    void *p = nullptr, *h = nullptr;
    int rc = tally_dev_alloc(ix, t->cap * 32, &p);
    if (rc) return rc;
    if ((rc = tally_dev_alloc(ix, 64, &h))) { tally_dev_free(ix, p); return rc; }
    t->slots = static_cast<uint64_t *>(p);
    t->hdr = static_cast<uint64_t *>(h);
    rc = rbg_tally_reset(t.get());
    if (rc) { tally_dev_free(ix, p); tally_dev_free(ix, h); return rc; }
    *out = t.release();
    return RBG_OK;
    });
}

void rbg_tally_free(rbg_tally *t) {
    if (!t) return;
    (void)guarded([&]() -> int {
    DeviceScope scope(t->ix->device);
    (void)hipDeviceSynchronize();
    tally_dev_free(t->ix, t->slots);
    tally_dev_free(t->ix, t->hdr);
    tally_dev_free(t->ix, t->ws);
    tally_dev_free(t->ix, t->xhdr);
    delete t;
    return RBG_OK;
    });
}

int rbg_tally_reset(rbg_tally *t) {
    return guarded([&]() -> int {
    if (!t) return RBG_EARG;
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = hipStreamPerThread;
    if (launch_tally_clear(t->slots, t->cap, st)) return RBG_ENODEV;
    HIP_TRY(hipMemsetAsync(t->hdr, 0, 64, st));
    if (t->xhdr) HIP_TRY(hipMemsetAsync(t->xhdr, 0, 32, st));
    HIP_TRY(hipStreamSynchronize(st));
    t->reads = 0;
    t->bound = 0;
    t->grows = 0;
    return RBG_OK;
    });
}

int rbg_tally_reserve(rbg_tally *t, uint64_t extra) {
    return guarded([&]() -> int {
    if (!t) return RBG_EARG;
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    return tally_reserve(t, extra);
    });
}

size_t rbg_tally_add_tmp_bytes(uint64_t R) { return tally_melem_bytes(R) + scan_tmp_bytes(R); }

int rbg_tally_add_dev(rbg_tally *t, const rbg_report_seed_t *d_recs, uint64_t R, const uint64_t *d_mk, uint64_t M_upper, void *d_tmp, size_t tmp_bytes,
                      void *stream) {
    return guarded([&]() -> int {
    if (!t) return RBG_EARG;
    if (R == 0) return RBG_OK;
    if (!d_recs || !d_tmp || (R >> 32) || (M_upper && !d_mk) || tmp_bytes < rbg_tally_add_tmp_bytes(R) || (reinterpret_cast<uintptr_t>(d_tmp) & 7)) return RBG_EARG;
    if (M_upper > tally_room(t)) return RBG_EARG;   // rbg_tally_reserve first: nothing is launched into a table that could fill up
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    uint64_t *melem = static_cast<uint64_t *>(d_tmp);
    if (launch_report_melem(d_recs, R, melem, static_cast<char *>(d_tmp) + tally_melem_bytes(R), tmp_bytes - tally_melem_bytes(R), stream)) return RBG_ENODEV;
    return tally_add_mapped(t, d_recs, R, d_mk, melem, M_upper, static_cast<hipStream_t>(stream));
    });
}

size_t rbg_tally_add_reads_tmp_bytes(uint64_t N, uint64_t R) { return tally_melem_bytes(R) + tally_span_bytes(R) + scan_tmp_bytes(R); }

int rbg_tally_add_reads_dev(rbg_tally *t, const rbg_report_seed_t *d_recs, uint64_t R, const uint64_t *d_rep_off, uint64_t N, const uint64_t *d_mk, uint64_t M_upper,
                            uint32_t tally_flags, void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!t || !tally_flags_ok(tally_flags)) return RBG_EARG;
    if (R == 0 || N == 0) {   // nothing to add; reads without printed records are still reads seen
        if (tally_flags & RBG_TALLY_PER_READ) t->reads += N;
        return RBG_OK;
    }
    if (!d_recs || !d_tmp || (R >> 32) || (M_upper && !d_mk) || tmp_bytes < rbg_tally_add_reads_tmp_bytes(N, R) || (reinterpret_cast<uintptr_t>(d_tmp) & 7)) return RBG_EARG;
    if ((tally_flags & RBG_TALLY_PER_READ) && !d_rep_off) return RBG_EARG;
    if (M_upper > tally_room(t)) return RBG_EARG;   // rbg_tally_reserve first, as for rbg_tally_add_dev
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    char *tmp = static_cast<char *>(d_tmp);   // melem | the records' read spans | the scan's temporaries
    const size_t used = tally_melem_bytes(R) + tally_span_bytes(R);
    uint64_t *melem = reinterpret_cast<uint64_t *>(tmp);
    if (launch_report_melem(d_recs, R, melem, tmp + used, tmp_bytes - used, stream)) return RBG_ENODEV;
    return tally_add_mapped(t, d_recs, R, d_mk, melem, M_upper, static_cast<hipStream_t>(stream), tally_flags, d_rep_off, N, tmp + tally_melem_bytes(R));
    });
}

int rbg_tally_add_entries(rbg_tally *t, const rbg_tally_entry_t *entries, uint64_t count) {
    return guarded([&]() -> int {
    if (!t || (count && !entries)) return RBG_EARG;
    if (count == 0) return RBG_OK;
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    int rc = tally_reserve(t, count);
    if (rc) return rc;
    DevBuf din;
    if ((rc = din.alloc(count * sizeof(rbg_tally_entry_t)))) return rc;
    hipStream_t st = hipStreamPerThread;
    HIP_TRY(hipMemcpyAsync(din.p, entries, count * sizeof(rbg_tally_entry_t), hipMemcpyHostToDevice, st));
    if (launch_tally_add_entries(t->slots, t->cap, t->hdr, din.p, count, st)) return RBG_ENODEV;
    HIP_TRY(hipStreamSynchronize(st));
    t->bound += count;
    return RBG_OK;
    });
}

int rbg_tally_export(rbg_tally *t, uint64_t *count, rbg_tally_entry_t **entries) {
    return guarded([&]() -> int {
    if (!t || !count || !entries) return RBG_EARG;
    *count = 0;
    *entries = nullptr;
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = hipStreamPerThread;
    DevBuf dpos, dtmp, dout;
    const size_t tmp_bytes = tally_compact_tmp_bytes(t->cap);
    int rc;
    if ((rc = dpos.alloc((t->cap + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
    if (launch_tally_compact_plan(t->slots, t->cap, dpos.as<uint64_t>(), dtmp.p, tmp_bytes, st)) return RBG_ENODEV;
    uint64_t live = 0, hdr[8];
    HIP_TRY(hipMemcpyAsync(&live, dpos.as<uint64_t>() + t->cap, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hdr, t->hdr, 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t n = live + (hdr[1] + hdr[2] ? 1 : 0);
    auto *h = static_cast<rbg_tally_entry_t *>(alloc_result(n * sizeof(rbg_tally_entry_t)));
    if (!h) return RBG_ENOMEM;
    if (n) {
        if ((rc = dout.alloc((live + 1) * sizeof(rbg_tally_entry_t)))) { rbg_free_buffer(h); return rc; }
        if (launch_tally_compact_fill(t->slots, t->cap, t->hdr, dpos.as<uint64_t>(), dout.p, st)) { rbg_free_buffer(h); return RBG_ENODEV; }
        if ((rc = d2h_result(h, dout.p, n * sizeof(rbg_tally_entry_t), st))) { rbg_free_buffer(h); return rc; }
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { rbg_free_buffer(h); return RBG_ENODEV; }
        // (sequence, position, allele) is the numeric order of rotl64(marker, 4) (k_report.hip); the array is the size of the distinct marker set
        std::sort(h, h + n, [](const rbg_tally_entry_t &a, const rbg_tally_entry_t &b) { return tally_rotl4(a.marker) < tally_rotl4(b.marker); });
    }
    *count = n;
    *entries = h;
    return RBG_OK;
    });
}

int rbg_tally_info(rbg_tally *t, uint64_t out[6]) {
    return guarded([&]() -> int {
    if (!t || !out) return RBG_EARG;
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    HIP_TRY(hipDeviceSynchronize());
    uint64_t hdr[8];
    HIP_TRY(hipMemcpy(hdr, t->hdr, 64, hipMemcpyDeviceToHost));
    out[0] = hdr[5] + (hdr[1] + hdr[2] ? 1 : 0);
    out[1] = t->cap;
    out[2] = t->grows;
    out[3] = hdr[6];
    out[4] = hdr[7];
    out[5] = hdr[4];
    return RBG_OK;
    });
}

int rbg_tally_read_info(rbg_tally *t, uint64_t out[4]) {
    return guarded([&]() -> int {
    if (!t || !out) return RBG_EARG;
    out[0] = t->reads;
    out[1] = out[2] = out[3] = 0;
    if (!t->xhdr) return RBG_OK;   // (no per-read add with records yet)
    DeviceScope scope(t->ix->device);
    if (scope.rc) return scope.rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out + 1, t->xhdr + 1, 24, hipMemcpyDeviceToHost));
    return RBG_OK;
    });
}

}  // extern "C"
