// capi/build_text.ipp -- an index from its text (sa_build.hip): the suffix array and the BWT's runs on the device (rbg_suffix_array_dev, rbg_text_runs_*_dev,
// rbg_sa_info; no handle, the current device, like rbg_sample_reads_dev), and the host calls that go from a text in host memory to a handle
// (rbg_build_from_text) or to the cache file (rbg_convert_text) along rbg_build_from_runs' / rbg_convert_runs_markers' own path.  Part of rbg_capi.hip.
namespace {
std::mutex g_sa_info_mu;
uint64_t g_sa_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};

// 4 or 8 for a text of n symbols under RBG_OPT_POS_BYTES (the rule of a load: load.ipp)
uint32_t text_pos_bytes(const uint64_t n) { return (g_opt_pos_bytes.load() == 8 || n >= 0xFFFFFFF0ull) ? 8 : 4; }
bool pos_bytes_ok(const uint64_t n, const uint32_t pos_bytes) { return pos_bytes == 8 || (pos_bytes == 4 && n < 0xFFFFFFF0ull); }

// what rbg_build_from_text holds on the device at its peak: the text, the suffix array and the larger of the two scratch areas
uint64_t text_build_bytes(const uint64_t n, const uint32_t pos_bytes) {
    return n + n * pos_bytes + std::max<uint64_t>(sa_tmp_bytes(n, pos_bytes), text_runs_tmp_bytes(n, pos_bytes)) + 3 * 256;
}

struct TextRuns {
    std::vector<uint8_t> heads;
    std::vector<uint64_t> lens, ssa, esa;
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

// the text's run arrays, through the device
int text_to_runs(const uint8_t *text, const uint64_t n, const int device, TextRuns &out) {
    if (device == RBG_DEVICE_NONE) return RBG_ENODEV;
    if (n == 0) return RBG_EARG;
    DeviceScope scope(device);
    if (scope.rc) return scope.rc;
    const uint32_t pb = text_pos_bytes(n);
    // the formula against the device before anything is allocated: no allocation fails half-way
    if (n > (uint64_t(1) << 56)) return RBG_ENOMEM;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (text_build_bytes(n, pb) > free_b) return RBG_ENOMEM;
    if (!text) return RBG_EARG;
    hipStream_t st = hipStreamPerThread;
    const size_t tmp_bytes = std::max(sa_tmp_bytes(n, pb), text_runs_tmp_bytes(n, pb));
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
    return RBG_OK;
}
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

int rbg_build_from_text(const uint8_t *text, uint64_t n, int flags, int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!out) return RBG_EARG;
    *out = nullptr;
    TextRuns t;
    int rc = text_to_runs(text, n, device, t);
    if (rc) return rc;
    const bool sa = (flags & RBG_LOAD_SA) != 0;
    return rbg_build_from_runs(t.heads.data(), t.lens.data(), t.heads.size(), sa ? t.ssa.data() : nullptr, sa ? t.esa.data() : nullptr, device, out);
    });
}

int rbg_convert_text(const uint8_t *text, uint64_t n, const char *docs_text, int flags, int device, const char *out_path) {
    return guarded([&]() -> int {
    if (!out_path) return RBG_EARG;
    TextRuns t;
    int rc = text_to_runs(text, n, device, t);
    if (rc) return rc;
    const bool sa = (flags & RBG_LOAD_SA) != 0;
    return rbg_convert_runs_markers(t.heads.data(), t.lens.data(), t.heads.size(), sa ? t.ssa.data() : nullptr, sa ? t.esa.data() : nullptr, nullptr, nullptr, 0,
                                    nullptr, nullptr, docs_text, out_path);
    });
}

}  // extern "C"
