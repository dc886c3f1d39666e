// capi/fl.ipp -- the FL index on the handle's device (rbg_fl_prepare, rbg_fl_info; rbg_fl.hpp: the structure, its builder and its step), FL of rows
// (rbg_fl_dev) and the right extension of located seeds by an FL walk (rbg_extend_right_dev; fl_extend.hip).  rbg_align_sam_extend_both is in sam.ipp.  Part of
// rbg_capi.hip.
namespace {
bool fl_ready(const rbg_index *ix) { return ix->fl_dev.blob != nullptr; }

uint32_t sam_grid_cap_env() {
    const char *e = std::getenv("RBG_SAM_GRID_CAP");
    const long long v = e && *e ? std::atoll(e) : 0;
    return v > 0 && v < (1ll << 31) ? static_cast<uint32_t>(v) : 0u;
}

int fl_prepare(rbg_index *ix) {
    if (!queryable(ix)) return RBG_ENODEV;
    std::lock_guard<std::mutex> g(ix->mu);
    if (fl_ready(ix)) return RBG_OK;
    const HostIndex &h = ix->H();
    if (h.r == 0 || h.run_heads.size() != h.r || h.run_start.size() != h.r + 1) return RBG_ENOTLOADED;
    const auto t0 = std::chrono::steady_clock::now();
    FlIndex F;
    if (!fl_build(h.run_heads.data(), h.run_start.data(), h.r, h.f, h.pos_bytes, F)) return RBG_EARG;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    // (an allocation of its own, never a piece of the arena, tracked like rbg_docs_prepare's)
    void *p = nullptr;
    const size_t alloc = arena_round(std::max<size_t>(F.bytes(), 16));
    hipError_t e = hipMalloc(&p, alloc);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV;
    }
    ix->allocs.push_back({p, alloc});
    ix->hbm_bytes += alloc;
    if (F.bytes() && (e = hipMemcpy(p, F.blob.data(), F.bytes(), hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipGetLastError();
        free_tracked(ix, p);
        return RBG_ENODEV;
    }
    rbg_index::FlDev &v = ix->fl_dev;
    v.view = F.view(p);
    v.bytes = F.bytes();
    v.dir_entries = 0;
    for (uint32_t j = 0; j < kFlBases; ++j) { v.runs[j] = F.runs[j]; v.dir_entries += F.dir_entries[j]; }
    v.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    v.blob = p;
    return RBG_OK;
}
}  // namespace

extern "C" {

int rbg_fl_prepare(rbg_index *ix) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    return fl_prepare(ix);
    });
}

int rbg_fl_info(const rbg_index *ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return RBG_EARG;
    const rbg_index::FlDev &v = ix->fl_dev;
    out[0] = fl_ready(ix) ? 1 : 0;
    out[1] = v.bytes;
    uint64_t shifts = 0;
    for (uint32_t j = 0; j < kFlBases; ++j) { out[2 + j] = v.runs[j]; shifts |= static_cast<uint64_t>(v.view.shift[j] & 0xFFu) << (8 * j); }
    out[6] = shifts;
    out[7] = v.dir_entries;
    return RBG_OK;
    });
}

int rbg_fl_dev(rbg_index *ix, const uint64_t *d_rows, uint64_t M, uint8_t *d_sym, uint64_t *d_next, void *stream) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!fl_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!d_rows || !d_sym || !d_next)) return RBG_EARG;
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf derr;   // (released after the wait below: nothing of this call still runs on it)
    int rc = derr.alloc(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(derr.p, 0, 16, st));
    if (launch_fl_rows(ix->fl_dev.view, ix->H().pos_bytes, ix->H().n, d_rows, M, d_sym, d_next, derr.as<unsigned int>(), sam_grid_cap_env(), st)) return RBG_ENODEV;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return err ? RBG_EARG : RBG_OK;
    });
}

int rbg_extend_right_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, const uint32_t *d_item_seq, const uint32_t *d_item_b,
                         const uint64_t *d_item_row, const uint32_t *d_item_skip, const uint64_t *d_item_limit, uint64_t M, uint32_t max_mismatch,
                         rbg_extend_t *d_out, void *stream) {
    return guarded([&]() -> int {
    if (!ix || max_mismatch > RBG_SAM_MAX_MISMATCH) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!fl_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!d_seqs || !d_off || !d_item_seq || !d_item_b || !d_item_row || !d_item_skip || !d_item_limit || !d_out)) return RBG_EARG;
    if ((reinterpret_cast<uintptr_t>(d_seqs) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 3)) return RBG_EARG;   // reads are fetched as aligned 16-byte chunks
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf derr;
    int rc = derr.alloc(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(derr.p, 0, 16, st));
    if (launch_extend_right(ix->fl_dev.view, ix->H().pos_bytes, ix->H().n, d_seqs, d_off, N, d_item_seq, d_item_b, d_item_row, d_item_skip, d_item_limit, nullptr, M,
                            max_mismatch, d_out, derr.as<unsigned int>(), sam_grid_cap_env(), st))
        return RBG_ENODEV;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return err ? RBG_EARG : RBG_OK;
    });
}

}  // extern "C"
