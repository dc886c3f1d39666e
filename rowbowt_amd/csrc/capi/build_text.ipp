// capi/build_text.ipp -- an index from its text (sa_build.hip): the suffix array and the BWT's runs on the device (rbg_suffix_array_dev, rbg_text_runs_*_dev,
// rbg_sa_info; no handle, the current device, like rbg_sample_reads_dev), the marker array from site records over that suffix array (mk_build.hip:
// rbg_marker_runs_*_dev), and the host calls that go from a text in host memory to a handle (rbg_build_from_text, rbg_build_from_text_markers) or to the cache
// file (rbg_convert_text, rbg_convert_text_markers) along rbg_build_from_runs' / rbg_set_markers' / rbg_convert_runs_markers' own path.  Part of rbg_capi.hip.
namespace {
std::mutex g_sa_info_mu;
uint64_t g_sa_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// 4 or 8 for a text of n symbols under RBG_OPT_POS_BYTES (the rule of a load: load.ipp)
uint32_t text_pos_bytes(const uint64_t n) { return (g_opt_pos_bytes.load() == 8 || n >= 0xFFFFFFF0ull) ? 8 : 4; }
bool pos_bytes_ok(const uint64_t n, const uint32_t pos_bytes) { return pos_bytes == 8 || (pos_bytes == 4 && n < 0xFFFFFFF0ull); }

// the site records of rbg_build_from_text_markers (S == 0: none) and the marker array made from them
struct SiteRecords {
    const uint64_t *pos = nullptr, *first = nullptr, *val = nullptr;
    uint64_t S = 0;
    uint32_t w = 0;
};

// the one scratch area of the build: the largest of what the suffix array, the runs and (with records) the marker pass ask for
size_t text_scratch_bytes(const uint64_t n, const uint32_t pos_bytes, const SiteRecords &mk) {
    return std::max(std::max(sa_tmp_bytes(n, pos_bytes), text_runs_tmp_bytes(n, pos_bytes)), mk.S ? marker_runs_tmp_bytes(n, mk.S, mk.w) : size_t(0));
}

// what rbg_build_from_text holds on the device at its peak: the text, the suffix array, the scratch and the three record arrays
uint64_t text_build_bytes(const uint64_t n, const uint32_t pos_bytes, const SiteRecords &mk) {
    return n + n * pos_bytes + text_scratch_bytes(n, pos_bytes, mk) + 3 * 256 + (mk.S ? 24 * mk.S + 3 * 256 : 0);
}

struct TextRuns {
    std::vector<uint8_t> heads;
    std::vector<uint64_t> lens, ssa, esa;
    std::vector<uint64_t> mk_start, mk_end, mk_off, mk_vals;      // (with site records: the arguments of rbg_set_markers)
};

// a plain allocation that goes back when the call ends (gigabytes: not a block of the pool)
struct DevBlock {
    void *p = nullptr;
    int alloc(const size_t bytes) {
        const hipError_t e = hipMalloc(&p, bytes ? bytes : 8);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV;
        }
        return RBG_OK;
    }
    ~DevBlock() { if (p) (void)hipFree(p); }
};

int sa_rc(const int rc) { return rc == 0 ? RBG_OK : rc == 1 ? RBG_EARG : RBG_ENODEV; }

// the marker array of the records, with the suffix array still on the device; d_tmp is the build's scratch, free again
int text_markers(const void *d_sa, const uint64_t n, const uint32_t pb, const SiteRecords &mk, void *d_tmp, const size_t tmp_bytes, hipStream_t st, TextRuns &out) {
    DevBlock d_pos, d_first, d_val;
    int rc;
    if ((rc = d_pos.alloc(mk.S * 8)) || (rc = d_first.alloc(mk.S * 8)) || (rc = d_val.alloc(mk.S * 8))) return rc;
    HIP_TRY(hipMemcpyAsync(d_pos.p, mk.pos, mk.S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_first.p, mk.first, mk.S * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_val.p, mk.val, mk.S * 8, hipMemcpyHostToDevice, st));
    uint64_t nruns = 0, nvals = 0;
    rc = marker_runs_plan(d_sa, n, pb, static_cast<const uint64_t *>(d_pos.p), static_cast<const uint64_t *>(d_first.p), static_cast<const uint64_t *>(d_val.p), mk.S,
                          mk.w, d_tmp, tmp_bytes, &nruns, &nvals, st);
    if (rc) { (void)hipStreamSynchronize(st); return sa_rc(rc); }
    // the marker arrays (16 bytes per run, 8 per value; known only now), checked like the run arrays before any of them is allocated
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (16 * nruns + 8 * nvals + 8 + 4 * 256 > free_b) return RBG_ENOMEM;
    DevBlock d_start, d_end, d_off, d_vals;
    if ((rc = d_start.alloc(nruns * 8)) || (rc = d_end.alloc(nruns * 8)) || (rc = d_off.alloc((nruns + 1) * 8)) || (rc = d_vals.alloc(nvals * 8))) return rc;
    rc = marker_runs_fill(n, pb, static_cast<const uint64_t *>(d_val.p), mk.S, mk.w, d_tmp, tmp_bytes, nruns, nvals, static_cast<uint64_t *>(d_start.p),
                          static_cast<uint64_t *>(d_end.p), static_cast<uint64_t *>(d_off.p), static_cast<uint64_t *>(d_vals.p), st);
    if (rc) { (void)hipStreamSynchronize(st); return sa_rc(rc); }
    out.mk_start.resize(nruns);
    out.mk_end.resize(nruns);
    out.mk_off.resize(nruns + 1);
    out.mk_vals.resize(nvals);
    HIP_TRY(hipMemcpyAsync(out.mk_start.data(), d_start.p, nruns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out.mk_end.data(), d_end.p, nruns * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out.mk_off.data(), d_off.p, (nruns + 1) * 8, hipMemcpyDeviceToHost, st));
    if (nvals) HIP_TRY(hipMemcpyAsync(out.mk_vals.data(), d_vals.p, nvals * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RBG_OK;
}

// the text's run arrays, and with site records its marker array, through the device
int text_to_runs(const uint8_t *text, const uint64_t n, const int device, TextRuns &out, const SiteRecords &mk = SiteRecords()) {
    if (device == RBG_DEVICE_NONE) return RBG_ENODEV;
    if (n == 0) return RBG_EARG;
    if (mk.S && (!mk.pos || !mk.first || !mk.val || mk.w < 1 || mk.w > 64 || mk.S > n)) return RBG_EARG;
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    const uint32_t pb = text_pos_bytes(n);
    // the formula against the device before anything is allocated: no allocation fails half-way
    if (n > (uint64_t(1) << 56)) return RBG_ENOMEM;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (text_build_bytes(n, pb, mk) > free_b) return RBG_ENOMEM;
    if (!text) return RBG_EARG;
    hipStream_t st = hipStreamPerThread;
    const size_t tmp_bytes = text_scratch_bytes(n, pb, mk);
    DevBlock d_text, d_sa, d_tmp;
    int rc;
    if ((rc = d_text.alloc(n)) || (rc = d_sa.alloc(n * pb)) || (rc = d_tmp.alloc(tmp_bytes))) return rc;
    HIP_TRY(hipMemcpyAsync(d_text.p, text, n, hipMemcpyHostToDevice, st));
    uint64_t info[8];
    rc = sa_build(static_cast<const uint8_t *>(d_text.p), n, d_sa.p, pb, d_tmp.p, tmp_bytes, st, info);
    if (rc == 0 || rc == 1) {
        std::lock_guard<std::mutex> g(g_sa_info_mu);
        std::memcpy(g_sa_info, info, sizeof info);
    }
    if (rc) { (void)hipStreamSynchronize(st); return sa_rc(rc); }
    uint64_t R = 0;
    if ((rc = text_runs_plan(static_cast<const uint8_t *>(d_text.p), d_sa.p, n, pb, d_tmp.p, tmp_bytes, &R, st))) { (void)hipStreamSynchronize(st); return sa_rc(rc); }
    if (R == 0 || R > n) return RBG_ENODEV;
    {
        // the run arrays (25 bytes per run; r is known only now) beside the text, the suffix array and the scratch, which the fill still reads: checked as a
        // whole like the first three, so that none of the four is allocated when they do not fit together
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        if (25 * R + 4 * 256 > free_b) return RBG_ENOMEM;
        DevBlock d_heads, d_lens, d_ssa, d_esa;
        if ((rc = d_heads.alloc(R)) || (rc = d_lens.alloc(R * 8)) || (rc = d_ssa.alloc(R * 8)) || (rc = d_esa.alloc(R * 8))) return rc;
        rc = text_runs_fill(static_cast<const uint8_t *>(d_text.p), d_sa.p, n, pb, d_tmp.p, tmp_bytes, R, static_cast<uint8_t *>(d_heads.p),
                            static_cast<uint64_t *>(d_lens.p), static_cast<uint64_t *>(d_ssa.p), static_cast<uint64_t *>(d_esa.p), st);
        if (rc) { (void)hipStreamSynchronize(st); return sa_rc(rc); }
        out.heads.resize(R);
        out.lens.resize(R);
        out.ssa.resize(R);
        out.esa.resize(R);
        HIP_TRY(hipMemcpyAsync(out.heads.data(), d_heads.p, R, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.lens.data(), d_lens.p, R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.ssa.data(), d_ssa.p, R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out.esa.data(), d_esa.p, R * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }      // (the run arrays go back: the marker pass has the suffix array, the scratch and its own arrays)
    return mk.S ? text_markers(d_sa.p, n, pb, mk, d_tmp.p, tmp_bytes, st, out) : RBG_OK;
}

bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
}  // namespace

extern "C" {

size_t rbg_sa_tmp_bytes(uint64_t n, uint32_t pos_bytes) { return pos_bytes_ok(n, pos_bytes) ? sa_tmp_bytes(n, pos_bytes) : 0; }

int rbg_suffix_array_dev(const uint8_t *d_text, uint64_t n, void *d_sa, uint32_t pos_bytes, void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!d_text || !d_sa || !d_tmp || n == 0 || !pos_bytes_ok(n, pos_bytes)) return RBG_EARG;
    if (tmp_bytes < sa_tmp_bytes(n, pos_bytes) || (reinterpret_cast<uintptr_t>(d_tmp) & 255) || (reinterpret_cast<uintptr_t>(d_sa) & (pos_bytes - 1))) return RBG_EARG;
    uint64_t info[8];
    const int rc = sa_build(d_text, n, d_sa, pos_bytes, d_tmp, tmp_bytes, stream, info);
    if (rc == 0 || rc == 1) {
        std::lock_guard<std::mutex> g(g_sa_info_mu);
        std::memcpy(g_sa_info, info, sizeof info);
    }
    return sa_rc(rc);
    });
}

int rbg_sa_info(uint64_t out[8]) {
    return guarded([&]() -> int {
    if (!out) return RBG_EARG;
    std::lock_guard<std::mutex> g(g_sa_info_mu);
    std::memcpy(out, g_sa_info, sizeof g_sa_info);
    return RBG_OK;
    });
}

size_t rbg_text_runs_tmp_bytes(uint64_t n, uint32_t pos_bytes) { return pos_bytes_ok(n, pos_bytes) ? text_runs_tmp_bytes(n, pos_bytes) : 0; }

int rbg_text_runs_plan_dev(const uint8_t *d_text, const void *d_sa, uint64_t n, uint32_t pos_bytes, void *d_tmp, size_t tmp_bytes, uint64_t *R, void *stream) {
    return guarded([&]() -> int {
    if (!d_text || !d_sa || !d_tmp || !R || n == 0 || !pos_bytes_ok(n, pos_bytes)) return RBG_EARG;
    if (tmp_bytes < text_runs_tmp_bytes(n, pos_bytes) || (reinterpret_cast<uintptr_t>(d_tmp) & 255) || (reinterpret_cast<uintptr_t>(d_sa) & (pos_bytes - 1))) return RBG_EARG;
    return sa_rc(text_runs_plan(d_text, d_sa, n, pos_bytes, d_tmp, tmp_bytes, R, stream));
    });
}

int rbg_text_runs_fill_dev(const uint8_t *d_text, const void *d_sa, uint64_t n, uint32_t pos_bytes, const void *d_tmp, size_t tmp_bytes, uint64_t R,
                           uint8_t *d_heads, uint64_t *d_lens, uint64_t *d_ssa, uint64_t *d_esa, void *stream) {
    return guarded([&]() -> int {
    if (!d_text || !d_sa || !d_tmp || !d_heads || !d_lens || !d_ssa || !d_esa || n == 0 || R == 0 || R > n || !pos_bytes_ok(n, pos_bytes)) return RBG_EARG;
    if (tmp_bytes < text_runs_tmp_bytes(n, pos_bytes) || (reinterpret_cast<uintptr_t>(d_tmp) & 255) || (reinterpret_cast<uintptr_t>(d_sa) & (pos_bytes - 1))) return RBG_EARG;
    return sa_rc(text_runs_fill(d_text, d_sa, n, pos_bytes, d_tmp, tmp_bytes, R, d_heads, d_lens, d_ssa, d_esa, stream));
    });
}

size_t rbg_marker_runs_tmp_bytes(uint64_t n, uint64_t S, uint32_t w, uint32_t pos_bytes) {
    return pos_bytes_ok(n, pos_bytes) ? marker_runs_tmp_bytes(n, S, w) : 0;
}

int rbg_marker_runs_plan_dev(const void *d_sa, uint64_t n, uint32_t pos_bytes, const uint64_t *d_pos, const uint64_t *d_first, const uint64_t *d_val, uint64_t S,
                             uint32_t w, void *d_tmp, size_t tmp_bytes, uint64_t *nruns, uint64_t *nvals, void *stream) {
    return guarded([&]() -> int {
    if (!d_sa || !d_tmp || !nruns || !nvals || n == 0 || !pos_bytes_ok(n, pos_bytes) || (S && (!d_pos || !d_first || !d_val))) return RBG_EARG;
    const size_t need = marker_runs_tmp_bytes(n, S, w);
    if (need == 0 || tmp_bytes < need || (reinterpret_cast<uintptr_t>(d_tmp) & 255) || (reinterpret_cast<uintptr_t>(d_sa) & (pos_bytes - 1)) || !aligned8(d_pos) ||
        !aligned8(d_first) || !aligned8(d_val))
        return RBG_EARG;
    uint64_t r = 0, v = 0;
    const int rc = marker_runs_plan(d_sa, n, pos_bytes, d_pos, d_first, d_val, S, w, d_tmp, tmp_bytes, &r, &v, stream);
    if (rc == 0) *nruns = r, *nvals = v;
    return sa_rc(rc);
    });
}

int rbg_marker_runs_fill_dev(const void *d_sa, uint64_t n, uint32_t pos_bytes, const uint64_t *d_pos, const uint64_t *d_first, const uint64_t *d_val, uint64_t S,
                             uint32_t w, const void *d_tmp, size_t tmp_bytes, uint64_t nruns, uint64_t nvals, uint64_t *d_run_start, uint64_t *d_run_end,
                             uint64_t *d_mk_off, uint64_t *d_mk_vals, void *stream) {
    return guarded([&]() -> int {
    if (!d_sa || !d_tmp || !d_mk_off || n == 0 || !pos_bytes_ok(n, pos_bytes) || (S && (!d_pos || !d_first || !d_val)) || (nruns && (!d_run_start || !d_run_end)) ||
        (nvals && !d_mk_vals))
        return RBG_EARG;
    const size_t need = marker_runs_tmp_bytes(n, S, w);
    if (need == 0 || tmp_bytes < need || (reinterpret_cast<uintptr_t>(d_tmp) & 255) || (reinterpret_cast<uintptr_t>(d_sa) & (pos_bytes - 1)) || !aligned8(d_pos) ||
        !aligned8(d_first) || !aligned8(d_val) || !aligned8(d_run_start) || !aligned8(d_run_end) || !aligned8(d_mk_off) || !aligned8(d_mk_vals))
        return RBG_EARG;
    return sa_rc(marker_runs_fill(n, pos_bytes, d_val, S, w, d_tmp, tmp_bytes, nruns, nvals, d_run_start, d_run_end, d_mk_off, d_mk_vals, stream));
    });
}

int rbg_build_from_text_markers(const uint8_t *text, uint64_t n, const uint64_t *pos, const uint64_t *first, const uint64_t *val, uint64_t S, uint32_t w, int flags,
                                int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!out) return RBG_EARG;
    *out = nullptr;
    TextRuns t;
    SiteRecords mk;
    if (S) mk.pos = pos, mk.first = first, mk.val = val, mk.S = S, mk.w = w;
    int rc = text_to_runs(text, n, device, t, mk);
    if (rc) return rc;
    const bool sa = (flags & RBG_LOAD_SA) != 0;
    rc = rbg_build_from_runs(t.heads.data(), t.lens.data(), t.heads.size(), sa ? t.ssa.data() : nullptr, sa ? t.esa.data() : nullptr, device, out);
    if (rc || !S) return rc;
    if ((rc = rbg_set_markers(*out, t.mk_start.data(), t.mk_end.data(), t.mk_start.size(), t.mk_off.data(), t.mk_vals.data()))) {
        rbg_free(*out);
        *out = nullptr;
    }
    return rc;
    });
}

int rbg_build_from_text(const uint8_t *text, uint64_t n, int flags, int device, rbg_index **out) {
    return rbg_build_from_text_markers(text, n, nullptr, nullptr, nullptr, 0, 0, flags, device, out);
}

int rbg_convert_text_markers(const uint8_t *text, uint64_t n, const uint64_t *pos, const uint64_t *first, const uint64_t *val, uint64_t S, uint32_t w,
                             const char *docs_text, int flags, int device, const char *out_path) {
    return guarded([&]() -> int {
    if (!out_path) return RBG_EARG;
    TextRuns t;
    SiteRecords mk;
    if (S) mk.pos = pos, mk.first = first, mk.val = val, mk.S = S, mk.w = w;
    int rc = text_to_runs(text, n, device, t, mk);
    if (rc) return rc;
    const bool sa = (flags & RBG_LOAD_SA) != 0;
    return rbg_convert_runs_markers(t.heads.data(), t.lens.data(), t.heads.size(), sa ? t.ssa.data() : nullptr, sa ? t.esa.data() : nullptr,
                                    S ? t.mk_start.data() : nullptr, S ? t.mk_end.data() : nullptr, t.mk_start.size(), S ? t.mk_off.data() : nullptr,
                                    S ? t.mk_vals.data() : nullptr, docs_text, out_path);
    });
}

int rbg_convert_text(const uint8_t *text, uint64_t n, const char *docs_text, int flags, int device, const char *out_path) {
    return rbg_convert_text_markers(text, n, nullptr, nullptr, nullptr, 0, 0, docs_text, flags, device, out_path);
}

}  // extern "C"
