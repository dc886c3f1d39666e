// capi/extract.ipp -- the ISA sample on the handle's device (rbg_extract_prepare, rbg_extract_info; rbg_isa.hpp: the structure, its builder and its lookup),
// the rows of text positions (rbg_isa_dev) and the text of intervals (rbg_extract_dev, rbg_extract; extract.hip).  Part of rbg_capi.hip.
namespace {
bool isa_ready(const rbg_index *ix) { return ix->isa_dev.blob != nullptr && ix->fl_dev.blob != nullptr; }

int extract_prepare(rbg_index *ix) {
    if (!queryable(ix)) return RBG_ENODEV;
    {
        const HostIndex &h = ix->H();
        if (!h.has_tsa || h.r == 0 || h.run_heads.size() != h.r || h.run_start.size() != h.r + 1 || h.samples_last.size() != h.r || h.pred_pos.size() != h.r ||
            h.phi_base.size() != h.r)
            return RBG_ENOTLOADED;
    }
    int rc = fl_prepare(ix);      // (takes the handle's lock itself)
    if (rc) return rc;
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->isa_dev.blob) return RBG_OK;
    const HostIndex &h = ix->H();
    const auto t0 = std::chrono::steady_clock::now();
    IsaIndex I;
    if (!isa_build(h.run_heads.data(), h.run_start.data(), h.r, h.samples_last.data(), h.pred_pos.data(), h.phi_base.data(), h.pos_bytes, I)) return RBG_EARG;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    // (an allocation of its own, never a piece of the arena, tracked like rbg_fl_prepare's)
    void *p = nullptr;
    const size_t alloc = arena_round(std::max<size_t>(I.bytes(), 16));
    hipError_t e = hipMalloc(&p, alloc);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV;
    }
    ix->allocs.push_back({p, alloc});
    ix->hbm_bytes += alloc;
    if ((e = hipMemcpy(p, I.blob.data(), I.bytes(), hipMemcpyHostToDevice)) != hipSuccess) {
        (void)hipGetLastError();
        free_tracked(ix, p);
        return RBG_ENODEV;
    }
    rbg_index::IsaDev &v = ix->isa_dev;
    v.view = I.view(p);
    v.bytes = I.bytes();
    v.samples = I.samples;
    v.dir_entries = I.dir_entries;
    v.second_kind = I.second_kind;
    v.max_gap = I.max_gap;
    v.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    v.blob = p;
    return RBG_OK;
}

// the error word of an extract.hip launch as a return code
int extract_err(const uint32_t err) { return (err & 1u) ? RBG_EARG : (err & 2u) ? RBG_EFORMAT : RBG_OK; }

int extract_dev(rbg_index *ix, const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_out_off, uint64_t M, uint8_t *d_out, uint32_t *d_got,
                hipStream_t st) {
    DevBuf derr;   // (released after the wait below: nothing of this call still runs on it)
    int rc = derr.alloc(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(derr.p, 0, 16, st));
    if (launch_extract(ix->fl_dev.view, ix->isa_dev.view, ix->H().pos_bytes, d_pos, d_len, d_out_off, M, d_out, d_got, derr.as<unsigned int>(), sam_grid_cap_env(), st))
        return RBG_ENODEV;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return extract_err(err);
}
}  // namespace

extern "C" {

int rbg_extract_prepare(rbg_index *ix) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    return extract_prepare(ix);
    });
}

int rbg_extract_info(const rbg_index *ix, uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!ix || !out) return RBG_EARG;
    const rbg_index::IsaDev &v = ix->isa_dev;
    out[0] = isa_ready(ix) ? 1 : 0;
    out[1] = v.bytes;
    out[2] = v.samples;
    out[3] = v.view.shift;
    out[4] = v.dir_entries;
    out[5] = v.second_kind;
    out[6] = v.max_gap;
    out[7] = static_cast<uint64_t>(v.build_ms * 1000.0);
    return RBG_OK;
    });
}

int rbg_isa_dev(rbg_index *ix, const uint64_t *d_pos, uint64_t M, uint64_t *d_row, void *stream) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!isa_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!d_pos || !d_row)) return RBG_EARG;
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf derr;
    int rc = derr.alloc(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(derr.p, 0, 16, st));
    if (launch_isa_rows(ix->fl_dev.view, ix->isa_dev.view, ix->H().pos_bytes, d_pos, M, d_row, derr.as<unsigned int>(), sam_grid_cap_env(), st)) return RBG_ENODEV;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return extract_err(err);
    });
}

int rbg_isa(rbg_index *ix, const uint64_t *pos, uint64_t M, uint64_t *row) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!isa_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!pos || !row)) return RBG_EARG;
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    DevBuf d_pos, d_row;
    int rc;
    if ((rc = d_pos.alloc(M * 8)) || (rc = d_row.alloc(M * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(d_pos.p, pos, M * 8, hipMemcpyHostToDevice, st));
    rc = rbg_isa_dev(ix, d_pos.as<uint64_t>(), M, d_row.as<uint64_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(row, d_row.p, M * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBG_OK;
    });
}

int rbg_extract_dev(rbg_index *ix, const uint64_t *d_pos, const uint32_t *d_len, const uint64_t *d_out_off, uint64_t M, uint8_t *d_out, uint32_t *d_got,
                    void *stream) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!isa_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!d_pos || !d_len || !d_out_off || !d_out || !d_got)) return RBG_EARG;
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    return extract_dev(ix, d_pos, d_len, d_out_off, M, d_out, d_got, static_cast<hipStream_t>(stream));
    });
}

int rbg_extract(rbg_index *ix, const uint64_t *pos, const uint64_t *len, uint64_t M, uint8_t *out, uint64_t *got) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!isa_ready(ix)) return RBG_ENOTLOADED;
    if (M && (!pos || !len || !got)) return RBG_EARG;
    if (M == 0) return RBG_OK;
    const uint64_t n = ix->H().n, chunk = static_cast<uint64_t>(g_opt_extract_chunk.load());
    // the pieces: every interval cut into stretches of at most `chunk` bases, each an item of its own (nothing lies at or beyond n: what an interval asks
    // for there stays zero, as it does behind the terminator)
    uint64_t total = 0, pieces = 0;
    for (uint64_t i = 0; i < M; ++i) {
        if (pos[i] >= n) return RBG_EARG;
        if (total + len[i] < total) return RBG_EARG;
        total += len[i];
        pieces += (std::min(len[i], n - pos[i]) + chunk - 1) / chunk;
    }
    if (total && !out) return RBG_EARG;
    for (uint64_t i = 0; i < M; ++i) got[i] = 0;
    if (pieces == 0) return RBG_OK;
    std::vector<uint64_t> p_pos(pieces), p_off(pieces);
    std::vector<uint32_t> p_len(pieces), p_got(pieces);
    for (uint64_t i = 0, at = 0, j = 0; i < M; at += len[i], ++i)
        for (uint64_t d = 0, L = std::min(len[i], n - pos[i]); d < L; d += chunk, ++j) {
            p_pos[j] = pos[i] + d;
            p_off[j] = at + d;
            p_len[j] = static_cast<uint32_t>(std::min(chunk, L - d));
        }
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    DevBuf d_pos, d_off, d_len, d_got, d_out;
    int rc;
    if ((rc = d_pos.alloc(pieces * 8)) || (rc = d_off.alloc(pieces * 8)) || (rc = d_len.alloc(pieces * 4)) || (rc = d_got.alloc(pieces * 4)) ||
        (rc = d_out.alloc(total)))
        return rc;
    HIP_TRY(hipMemcpyAsync(d_pos.p, p_pos.data(), pieces * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off.p, p_off.data(), pieces * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_len.p, p_len.data(), pieces * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, total, st));
    rc = extract_dev(ix, d_pos.as<uint64_t>(), d_len.as<uint32_t>(), d_off.as<uint64_t>(), pieces, d_out.as<uint8_t>(), d_got.as<uint32_t>(), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p_got.data(), d_got.p, pieces * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // an interval ends at its first short piece: what later pieces found behind it is taken back, so the result never depends on the chunk
    for (uint64_t i = 0, at = 0, j = 0; i < M; at += len[i], ++i) {
        bool ended = false;
        for (uint64_t d = 0, L = std::min(len[i], n - pos[i]); d < L; d += chunk, ++j) {
            if (ended) continue;
            got[i] += p_got[j];
            ended = p_got[j] < p_len[j];
        }
        if (ended) std::memset(out + at + got[i], 0, len[i] - got[i]);
    }
    return RBG_OK;
    });
}

}  // extern "C"
