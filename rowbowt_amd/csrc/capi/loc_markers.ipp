// capi/loc_markers.ipp -- markers at located text positions (rb_locs' path): the marker table keyed by text position, the device pair over K3's
// output (k_loc_markers.hip) and the host calls above it.  Part of rbg_capi.hip.
namespace {
// plan + fill over arrays already on the device, the result copied out: the tail of both host calls below
int loc_markers_tail(rbg_index *ix, const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, uint64_t N, uint64_t *mk_off, uint64_t **mk,
                     hipStream_t st) {
    DevBuf dmoff, dtmp;
    const size_t tmp_bytes = scan_tmp_bytes(N);
    const int group = loc_markers_group();
    int rc;
    if ((rc = dmoff.alloc((N + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
    if (launch_loc_markers_plan(ix->dev, ix->cfg, d_locs, d_loc_off, d_off, N, dmoff.as<uint64_t>(), dtmp.p, tmp_bytes, group, st)) return RBG_ENODEV;
    return ragged_finish(N, dmoff, mk_off, mk, st, [&](uint64_t *d_vals) {
        return launch_loc_markers_fill(ix->dev, ix->cfg, d_locs, d_loc_off, d_off, N, dmoff.as<uint64_t>(), d_vals, group, st) ? RBG_ENODEV : RBG_OK;
    });
}
}  // namespace

extern "C" {

int rbg_set_text_markers(rbg_index *ix, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns, const uint64_t *mk_off,
                         const uint64_t *mk_vals) {
    return guarded([&]() -> int {
    if (!ix || !mk_off || (nruns && (!run_start || !run_end)) || (!mk_vals && mk_off[nruns])) return RBG_EARG;
    if (!markers_valid(run_start, run_end, nruns, mk_off)) return RBG_EARG;
    if (ix->primary) return RBG_EARG;    // attach to the primary, before rbg_replicate
    if (!queryable(ix)) return RBG_ENODEV;
    if (nruns && run_end[nruns - 1] >= ix->H().n) return RBG_EARG;   // text positions: [0, n)
    RawMarkers m;
    m.start.assign(run_start, run_start + nruns);
    m.end.assign(run_end, run_end + nruns);
    m.off.assign(mk_off, mk_off + nruns + 1);
    m.vals.assign(mk_vals, mk_vals + mk_off[nruns]);
    std::lock_guard<std::mutex> g(ix->mu);
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    return upload_text_markers(ix, m);
    });
}

// <prefix>.midx: the reference's rle_window_arr (rb_markers_tsa.cpp:99-101), read with the .mab parser -- see include/rbg.h on why that is an inference
int rbg_load_text_markers(rbg_index *ix, const char *path) {
    return guarded([&]() -> int {
    if (!ix || !path) return RBG_EARG;
    RawMarkers m;
    int rc = parse_mab(path, m);
    if (rc) return rc;
    if (m.end.size() != m.start.size() || m.off.size() != m.start.size() + 1 || m.off.back() != m.vals.size()) return RBG_EFORMAT;
    if (!markers_valid(m.start.data(), m.end.data(), m.start.size(), m.off.data())) return RBG_EFORMAT;
    return rbg_set_text_markers(ix, m.start.data(), m.end.data(), m.start.size(), m.off.data(), m.vals.data());
    });
}

size_t rbg_loc_markers_tmp_bytes(uint64_t N) { return scan_tmp_bytes(N); }

int rbg_loc_markers_plan_dev(rbg_index *ix, const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, uint64_t N, uint64_t *d_mk_off,
                             void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->has_tmk) return RBG_ENOTLOADED;
    if (!d_mk_off || (N && (!d_locs || !d_loc_off || !d_off || !d_tmp))) return RBG_EARG;
    if (tmp_bytes < scan_tmp_bytes(N)) return RBG_EARG;
    return launch_loc_markers_plan(ix->dev, ix->cfg, d_locs, d_loc_off, d_off, N, d_mk_off, d_tmp, tmp_bytes, loc_markers_group(), stream) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_loc_markers_fill_dev(rbg_index *ix, const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, uint64_t N,
                             const uint64_t *d_mk_off, uint64_t *d_mk, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->has_tmk) return RBG_ENOTLOADED;
    if (N && (!d_locs || !d_loc_off || !d_off || !d_mk_off || !d_mk)) return RBG_EARG;
    return launch_loc_markers_fill(ix->dev, ix->cfg, d_locs, d_loc_off, d_off, N, d_mk_off, d_mk, loc_markers_group(), stream) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_markers_at_locs(rbg_index *ix, const uint64_t *locs, const uint64_t *loc_off, const uint64_t *off, uint64_t N, uint64_t *mk_off, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!mk_off || !mk) return RBG_EARG;
    *mk = nullptr;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->has_tmk) return RBG_ENOTLOADED;
    if (N && (!loc_off || !off)) return RBG_EARG;
    int rc;
    if ((rc = check_offsets(off, N)) || (rc = check_offsets(loc_off, N))) return rc;
    const uint64_t L = N ? loc_off[N] : 0;
    if (L && !locs) return RBG_EARG;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    DevBuf dlocs, dloff, doff;
    if ((rc = dlocs.alloc(L * 8)) || (rc = dloff.alloc((N + 1) * 8)) || (rc = doff.alloc((N + 1) * 8))) return rc;
    if (L) HIP_TRY(hipMemcpyAsync(dlocs.p, locs, L * 8, hipMemcpyHostToDevice, st));
    if (N) {
        HIP_TRY(hipMemcpyAsync(dloff.p, loc_off, (N + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(doff.p, off, (N + 1) * 8, hipMemcpyHostToDevice, st));
    }
    return loc_markers_tail(ix, dlocs.as<uint64_t>(), dloff.as<uint64_t>(), doff.as<uint64_t>(), N, mk_off, mk, st);
    });
}

// one read of rb_locs, batched (rb_markers_tsa.cpp:76-88): find_locs_greedy_seeding, then the markers over every location's text interval.  The
// locations stay on the device between the two (greedy_host, capi/seeds.ipp: the marker pair runs behind K3, before the locations are copied out).
int rbg_find_loc_markers_greedy_seeding(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length, uint64_t max_hits,
                                        uint64_t *loc_off, uint64_t **locs, uint64_t *mk_off, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!loc_off || !locs || !mk_off || !mk) return RBG_EARG;
    *locs = nullptr;
    *mk = nullptr;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->has_tmk) return RBG_ENOTLOADED;
    const AfterLocate after = [&](const uint64_t *d_locs, const uint64_t *d_loc_off, const uint64_t *d_off, hipStream_t st) {
        return loc_markers_tail(ix, d_locs, d_loc_off, d_off, N, mk_off, mk, st);
    };
    const int rc = greedy_host(ix, seqs, off, N, min_length, nullptr, nullptr, nullptr, nullptr, nullptr, true, max_hits, loc_off, locs, &after);
    if (rc) {
        rbg_free_buffer(*mk); *mk = nullptr;
        rbg_free_buffer(*locs); *locs = nullptr;
        return rc;
    }
    if (!*mk) {   // no location in the whole batch: K3's fill never ran, and every list is empty
        std::fill(mk_off, mk_off + N + 1, uint64_t(0));
        *mk = static_cast<uint64_t *>(alloc_result(0));
        if (!*mk) { rbg_free_buffer(*locs); *locs = nullptr; return RBG_ENOMEM; }
    }
    return RBG_OK;
    });
}

}  // extern "C"
