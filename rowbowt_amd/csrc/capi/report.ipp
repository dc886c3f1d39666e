// capi/report.ipp -- rb_markers' report on the device (k_report.hip): the device steps and the two host calls above them.  Part of rbg_capi.hip.
namespace {
constexpr uint32_t kReportFlags = RBG_REPORT_LMEM | RBG_REPORT_HEURISTIC | RBG_REPORT_BEST_STRAND | RBG_REPORT_CLEAR_CONFLICTING | RBG_REPORT_CLEAR_IDENTICAL;

// what the reference (rowbowt.hpp:346-349, :423-426) and rb_markers check before the first read
int report_params_ok(const rbg_report_params_t *P) {
    if (!P || (P->flags & ~kReportFlags)) return RBG_EARG;
    if (P->ftab_k && P->ftab_k - 1 > P->wsize) return RBG_EARG;
    if ((P->flags & RBG_REPORT_LMEM) && P->ftab_k == 0) return RBG_EARG;
    return RBG_OK;
}

// read bytes per device pass of the report calls: greedy seeds 64 MiB of reads, lmem seeds as many as make rbg_get_markers_lmems' chunk of records
// (two strands per read); RBG_REPORT_CHUNK=<read bytes> overrides both (tests force several passes with it)
uint64_t report_chunk_bytes(bool lmem) {
    const char *e = std::getenv("RBG_REPORT_CHUNK");
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    if (v) return v;
    return lmem ? std::max<uint64_t>(lmem_chunk_records() / 2, 1) : uint64_t(64) << 20;
}

// RBG_REPORT_TRACE=1: seconds per device step of the report calls (each step synchronised), summed over the process and printed at exit
struct ReportTrace {
    bool on = std::getenv("RBG_REPORT_TRACE") != nullptr;
    std::mutex mu;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t passes = 0, reads = 0, d2h = 0;
    ~ReportTrace() {
        if (on && passes)
            std::fprintf(stderr, "rbg_markers_report: %llu passes, %llu reads, %llu bytes copied out: copy in + strands %.4f s, plan %.4f, fill %.4f, canon %.4f, "
                                 "select %.4f, text %.4f, copy out %.4f, tally %.4f\n", static_cast<unsigned long long>(passes), static_cast<unsigned long long>(reads),
                         static_cast<unsigned long long>(d2h), t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
};
ReportTrace g_report_trace;

struct ReportOut {   // where a call's result goes
    // records
    uint64_t *seed_off = nullptr;
    std::vector<rbg_report_seed_t> recs;
    std::vector<uint64_t> mk;
    // text
    bool want_text = false;
    const char *name_base = nullptr;
    const uint64_t *name_begin = nullptr;
    const uint32_t *name_len = nullptr;
    char *text = nullptr;
    size_t text_cap = 0, text_len = 0;
    // tally: the printed records' markers are added on the device, nothing is copied out
    rbg_tally *tally = nullptr;
};

// room for `need` bytes in the call's pinned text buffer (what is there is kept; no copy is in flight when this is called)
int report_text_room(rbg_index *ix, ReportOut &o, size_t need, size_t hint) {
    if (o.text && need <= o.text_cap) return RBG_OK;
    char *p = nullptr;
    int rc = take_text_out(ix, std::max(need + need / 2, hint), &p);
    if (rc) return rc;
    size_t cap = 0;
    {
        std::lock_guard<std::mutex> g(ix->text_mu);
        cap = find_text_out(ix, p)->cap;
    }
    if (o.text) {
        std::memcpy(p, o.text, o.text_len);
        (void)rbg_release_text(ix, o.text);
    }
    o.text = p;
    o.text_cap = cap;
    return RBG_OK;
}

// reads [a, b) of the batch: strands -> seeds -> canon -> select -> records, text or tally
int report_pass(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t a, uint64_t b, uint64_t N, const uint8_t *first_fwd,
                const rbg_report_params_t &P, ReportOut &o, hipStream_t st) {
    const uint64_t n = b - a, bytes = off[b] - off[a];
    const bool lmem = (P.flags & RBG_REPORT_LMEM) != 0, last = b == N;
    int rc;
    double lap_t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto lap_from = std::chrono::steady_clock::now();
    auto lap = [&](int slot) {
        if (!g_report_trace.on) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        lap_t[slot] += std::chrono::duration<double>(now - lap_from).count();
        lap_from = now;
    };
    uint64_t d2h_bytes = 0;
    // the raw reads and their offsets (off[a] is not 0 in a later pass: the strand kernel subtracts it)
    DevBuf draw, doff, dcoin, dseq2, doff2;
    const uint64_t first16 = off[a] & ~uint64_t(15), raw_bytes = off[b] - first16;
    std::vector<uint64_t> roff(n + 1);
    for (uint64_t i = 0; i <= n; ++i) roff[i] = off[a + i] - first16;
    if ((rc = draw.alloc(((raw_bytes + 15) & ~uint64_t(15)) + 16)) || (rc = doff.alloc((n + 1) * 8)) || (rc = dseq2.alloc(((2 * bytes + 15) & ~uint64_t(15)) + 16)) ||
        (rc = doff2.alloc((2 * n + 1) * 8)))
        return rc;
    if (raw_bytes) HIP_TRY(hipMemcpyAsync(draw.p, seqs + first16, raw_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(doff.p, roff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    const uint8_t *d_coin = nullptr;
    if (first_fwd && (P.flags & RBG_REPORT_HEURISTIC)) {
        if ((rc = dcoin.alloc(n))) return rc;
        HIP_TRY(hipMemcpyAsync(dcoin.p, first_fwd + a, n, hipMemcpyHostToDevice, st));
        d_coin = dcoin.as<uint8_t>();
    }
    if (launch_read_strands(draw.as<uint8_t>(), doff.as<uint64_t>(), n, bytes, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), st)) return RBG_ENODEV;
    lap(0);
    // the seeds of the 2n sequences
    const uint64_t n2 = 2 * n;
    DevBuf dsoff, dmoff, dtmp, dlog, dseeds, dmk;
    const uint64_t *d_seed_off = nullptr;
    uint64_t S = 0, total_mk = 0;
    if (!lmem) {
        const size_t tmp_bytes = scan_tmp_bytes(n2);
        if ((rc = dsoff.alloc((n2 + 1) * 8)) || (rc = dmoff.alloc((n2 + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
        size_t log_bytes = seed_log_bytes(n2, ix->H().pos_bytes, kSeedLogSeedsDefault);
        if (dlog.alloc(log_bytes)) log_bytes = 0;
        if (launch_marker_seeds_plan(ix->dev, ix->cfg, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), n2, P.wsize, P.max_range, P.ftab_k, dsoff.as<uint64_t>(),
                                     dmoff.as<uint64_t>(), dtmp.p, tmp_bytes, st, log_bytes ? dlog.p : nullptr, log_bytes))
            return RBG_ENODEV;
        HIP_TRY(hipMemcpyAsync(&S, dsoff.as<uint64_t>() + n2, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&total_mk, dmoff.as<uint64_t>() + n2, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lap(1);
        if (S >> 32) return RBG_EARG;   // (a pass holds at most 64 MiB of reads)
        if (o.tally && (rc = tally_reserve(o.tally, total_mk))) return rc;   // (total_mk bounds the pass's elements from above: canon and select only drop)
        if ((rc = dseeds.alloc(S * sizeof(rbg_marker_seed_t))) || (rc = dmk.alloc(total_mk * 8))) return rc;
        if (S && launch_marker_seeds_fill(ix->dev, ix->cfg, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), n2, P.wsize, P.max_range, P.ftab_k, dsoff.as<uint64_t>(),
                                          dmoff.as<uint64_t>(), dseeds.as<uint64_t>(), dmk.as<uint64_t>(), st, log_bytes ? dlog.p : nullptr, log_bytes))
            return RBG_ENODEV;
        d_seed_off = dsoff.as<uint64_t>();
    } else {
        S = 2 * bytes;   // one record per end position of every strand
        if (S >> 32) return RBG_EARG;
        const size_t tmp_bytes = marker_lmems_tmp_bytes(S);
        if ((rc = dmoff.alloc((n2 + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
        if (launch_marker_lmems_plan(ix->dev, ix->cfg, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), n2, S, P.wsize, P.max_range, P.ftab_k, dmoff.as<uint64_t>(), dtmp.p,
                                     tmp_bytes, st))
            return RBG_ENODEV;
        HIP_TRY(hipMemcpyAsync(&total_mk, dmoff.as<uint64_t>() + n2, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lap(1);
        if (o.tally && (rc = tally_reserve(o.tally, total_mk))) return rc;
        if ((rc = dseeds.alloc(S * sizeof(rbg_marker_seed_t))) || (rc = dmk.alloc(total_mk * 8))) return rc;
        if (S && launch_marker_lmems_fill(ix->dev, ix->cfg, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), n2, S, P.wsize, P.max_range, P.ftab_k, dtmp.p,
                                          dseeds.as<uint64_t>(), dmk.as<uint64_t>(), st))
            return RBG_ENODEV;
        d_seed_off = doff2.as<uint64_t>();
    }
    lap(2);
    // canonical records
    DevBuf dctmp;
    const size_t ctmp_bytes = seed_canon_tmp_bytes(S);
    if ((rc = dctmp.alloc(ctmp_bytes))) return rc;
    const uint32_t cflags = (P.flags & RBG_REPORT_HEURISTIC) ? P.flags & (RBG_REPORT_CLEAR_CONFLICTING | RBG_REPORT_CLEAR_IDENTICAL) : 0;
    if (total_mk && launch_seed_canon(ix->cfg, dseeds.as<uint64_t>(), S, dmk.as<uint64_t>(), P.min_range, cflags, P.read_len, dctmp.p, ctmp_bytes, report_canon_group(), st))
        return RBG_ENODEV;
    lap(3);
    // the printed records of every read
    DevBuf drep, drecs, dread, dstmp, dmelem;
    const size_t stmp_bytes = scan_tmp_bytes(std::max<uint64_t>(n, S));
    if ((rc = drep.alloc((n + 1) * 8)) || (rc = drecs.alloc(S * sizeof(rbg_report_seed_t))) || (rc = dread.alloc(S * 4)) || (rc = dstmp.alloc(stmp_bytes)) ||
        (rc = dmelem.alloc((S + 1) * 8)))
        return rc;
    if (launch_report_select(dseeds.as<uint64_t>(), d_seed_off, doff2.as<uint64_t>(), n, d_coin, P.read_len, P.min_seed_len, P.flags, drep.as<uint64_t>(), drecs.p,
                             dread.as<uint32_t>(), dstmp.p, stmp_bytes, st))
        return RBG_ENODEV;
    uint64_t R = 0, M = 0;
    std::vector<uint64_t> rep_off;
    if (o.want_text || o.tally) {
        HIP_TRY(hipMemcpyAsync(&R, drep.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    } else {
        rep_off.resize(n + 1);
        HIP_TRY(hipMemcpyAsync(rep_off.data(), drep.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (!o.want_text && !o.tally) {
        R = rep_off[n];
        const uint64_t base = o.recs.size();
        for (uint64_t i = 0; i < n; ++i) o.seed_off[a + i + 1] = base + rep_off[i + 1];
    }
    lap(4);
    if (R) {
        if (launch_report_melem(drecs.p, R, dmelem.as<uint64_t>(), dstmp.p, stmp_bytes, st)) return RBG_ENODEV;
        if (o.tally) {   // (room was reserved above; the add is the pass's last launch and nothing comes back)
            if ((rc = tally_add_mapped(o.tally, drecs.p, R, dmk.as<uint64_t>(), dmelem.as<uint64_t>(), total_mk, st))) return rc;
            lap(7);
        } else {
            HIP_TRY(hipMemcpyAsync(&M, dmelem.as<uint64_t>() + R, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const uint64_t E = R + M;
            DevBuf dws;
            const size_t ws_bytes = report_text_ws_bytes(E);
            if ((rc = dws.alloc(ws_bytes))) return rc;
            if (launch_report_map(dmelem.as<uint64_t>(), R, E, dws.p, ws_bytes, st)) return RBG_ENODEV;
            if (!o.want_text) {
                DevBuf drecs2, ddense;
                if ((rc = drecs2.alloc(R * sizeof(rbg_report_seed_t))) || (rc = ddense.alloc(M * 8))) return rc;
                if (launch_report_gather(drecs.p, dmelem.as<uint64_t>(), dmk.as<uint64_t>(), R, E, dws.p, ws_bytes, drecs2.p, ddense.as<uint64_t>(), st)) return RBG_ENODEV;
                lap(5);
                const uint64_t rbase = o.recs.size(), mbase = o.mk.size();
                o.recs.resize(rbase + R);
                o.mk.resize(mbase + M);
                if ((rc = d2h_result(o.recs.data() + rbase, drecs2.p, R * sizeof(rbg_report_seed_t), st))) return rc;
                if (M && (rc = d2h_result(o.mk.data() + mbase, ddense.p, M * 8, st))) return rc;
                HIP_TRY(hipStreamSynchronize(st));
                if (mbase)
                    for (uint64_t r = rbase; r < rbase + R; ++r) { o.recs[r].mk_begin += mbase; o.recs[r].mk_end += mbase; }
                d2h_bytes = R * sizeof(rbg_report_seed_t) + M * 8 + (n + 1) * 8;
            } else {
                // the names of the pass, back to back
                std::vector<uint32_t> noff(n + 1);
                uint64_t name_bytes = 0;
                for (uint64_t i = 0; i < n; ++i) { noff[i] = static_cast<uint32_t>(name_bytes); name_bytes += o.name_len[a + i]; }
                if (name_bytes >> 32) return RBG_EARG;
                noff[n] = static_cast<uint32_t>(name_bytes);
                std::vector<char> blob(name_bytes + 1);
                parallel_for(n, [&](uint64_t x, uint64_t y, unsigned) {
                    for (uint64_t i = x; i < y; ++i) std::memcpy(blob.data() + noff[i], o.name_base + o.name_begin[a + i], o.name_len[a + i]);
                });
                DevBuf dnoff, dnames, dtext;
                if ((rc = dnoff.alloc((n + 1) * 4)) || (rc = dnames.alloc(name_bytes + 1))) return rc;
                HIP_TRY(hipMemcpyAsync(dnoff.p, noff.data(), (n + 1) * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(dnames.p, blob.data(), name_bytes + 1, hipMemcpyHostToDevice, st));
                if (launch_report_text_plan(drecs.p, dread.as<uint32_t>(), dmelem.as<uint64_t>(), dmk.as<uint64_t>(), R, E, dnames.as<char>(), dnoff.as<uint32_t>(), dws.p,
                                            ws_bytes, st))
                    return RBG_ENODEV;
                const uint64_t *p_at = nullptr;
                const uint32_t *p_len = nullptr;
                report_text_total_ptrs(dws.p, E, &p_at, &p_len);
                uint64_t last_at = 0;
                uint32_t last_len = 0;
                HIP_TRY(hipMemcpyAsync(&last_at, p_at, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(&last_len, p_len, 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));   // (the name blob has been copied too)
                const uint64_t total = last_at + last_len;
                if ((rc = dtext.alloc(total))) return rc;
                if (launch_report_text_fill(drecs.p, dread.as<uint32_t>(), dmelem.as<uint64_t>(), dmk.as<uint64_t>(), R, E, dnames.as<char>(), dnoff.as<uint32_t>(), dws.p,
                                            ws_bytes, total, dtext.as<char>(), st))
                    return RBG_ENODEV;
                lap(5);
                // (a first pass that is not the last sizes the buffer for the whole batch from its own text per read byte)
                const size_t hint = last || !bytes ? 0 : static_cast<size_t>(static_cast<double>(total) / static_cast<double>(bytes) * static_cast<double>(off[N] - off[0]) * 1.25);
                if ((rc = report_text_room(ix, o, o.text_len + total, hint))) return rc;
                char *dst = o.text + o.text_len;
                o.text_len += total;
                d2h_bytes = total;
                if (!last || g_report_trace.on) {
                    HIP_TRY(hipMemcpyAsync(dst, dtext.p, total, hipMemcpyDeviceToHost, st));
                    HIP_TRY(hipStreamSynchronize(st));
                } else {
                    // the last copy-out runs on the handle's copy stream behind the fill kernel; the caller returns at once and the text's reader
                    // waits (rbg_wait_text), as in rbg_align_text
                    std::lock_guard<std::mutex> g(ix->text_mu);
                    rbg_index::TextOut *t = find_text_out(ix, o.text);
                    hipError_t e = hipEventRecord(t->done, st);
                    if (e == hipSuccess) e = hipStreamWaitEvent(ix->text_copy_stream, t->done, 0);
                    if (e == hipSuccess) e = hipMemcpyAsync(dst, dtext.p, total, hipMemcpyDeviceToHost, ix->text_copy_stream);
                    if (e == hipSuccess) e = hipEventRecord(t->done, ix->text_copy_stream);
                    HIP_TRY(e);
                    t->pending = true;
                    t->d_text = dtext.p; t->d_cls = dtext.cls; t->d_dev = dtext.dev;
                    dtext.p = nullptr;   // (the record owns the device block until the copy has been waited for)
                }
            }
            lap(6);
        }
    }
    if (g_report_trace.on) {
        std::lock_guard<std::mutex> g(g_report_trace.mu);
        for (int j = 0; j < 8; ++j) g_report_trace.t[j] += lap_t[j];
        g_report_trace.passes += 1;
        g_report_trace.reads += n;
        g_report_trace.d2h += d2h_bytes;
    }
    return RBG_OK;
}

int report_run(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd, const rbg_report_params_t *params, ReportOut &o) {
    int rc = report_params_ok(params);
    if (rc) return rc;
    if (!queryable(ix)) return RBG_ENODEV;
    if (N && !off) return RBG_EARG;
    if ((rc = check_offsets(off, N))) return rc;
    if (N && off[N] && !seqs) return RBG_EARG;
    if (N == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    const uint64_t chunk = report_chunk_bytes((params->flags & RBG_REPORT_LMEM) != 0);
    for (uint64_t a = 0; a < N && !rc;) {
        uint64_t b = a + 1;   // reads [a, b): at least one, and as many whole ones as fit the chunk (and 2^31 records' worth at most)
        while (b < N && off[b + 1] - off[a] <= chunk && b - a < (uint64_t(1) << 28)) ++b;
        rc = report_pass(ix, seqs, off, a, b, N, first_fwd, *params, o, st);
        a = b;
    }
    if (rc && o.text) { (void)rbg_release_text(ix, o.text); o.text = nullptr; }
    return rc;
}
}  // namespace

extern "C" {

size_t rbg_read_strands_bytes(uint64_t total_bytes) { return ((2 * total_bytes + 15) & ~uint64_t(15)) + 16; }

int rbg_read_strands_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total_bytes, uint8_t *d_seqs2, uint64_t *d_off2,
                         void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!d_off2 || (N && (!d_off || !d_seqs2 || (total_bytes && !d_seqs)))) return RBG_EARG;
    if ((reinterpret_cast<uintptr_t>(d_seqs) & 15) || (reinterpret_cast<uintptr_t>(d_seqs2) & 15)) return RBG_EARG;
    return launch_read_strands(d_seqs, d_off, N, total_bytes, d_seqs2, d_off2, stream) ? RBG_ENODEV : RBG_OK;
    });
}

size_t rbg_marker_seeds_canon_tmp_bytes(uint64_t S) { return seed_canon_tmp_bytes(S); }

int rbg_marker_seeds_canon_dev(rbg_index *ix, rbg_marker_seed_t *d_seeds, uint64_t S, uint64_t *d_mk, uint64_t min_range, uint32_t flags, uint64_t read_len,
                               void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (S == 0) return RBG_OK;
    if (!d_seeds || !d_mk || !d_tmp || (S >> 32) || tmp_bytes < seed_canon_tmp_bytes(S) || (reinterpret_cast<uintptr_t>(d_tmp) & 3)) return RBG_EARG;
    return launch_seed_canon(ix->cfg, reinterpret_cast<uint64_t *>(d_seeds), S, d_mk, min_range, flags & (RBG_REPORT_CLEAR_CONFLICTING | RBG_REPORT_CLEAR_IDENTICAL),
                             read_len, d_tmp, tmp_bytes, report_canon_group(), stream) ? RBG_ENODEV : RBG_OK;
    });
}

size_t rbg_report_select_tmp_bytes(uint64_t N) { return scan_tmp_bytes(N); }

int rbg_report_select_dev(rbg_index *ix, const rbg_marker_seed_t *d_seeds, const uint64_t *d_seed_off, const uint64_t *d_off2, uint64_t N,
                          const uint8_t *d_first_fwd, const rbg_report_params_t *params, uint64_t *d_rep_off, rbg_report_seed_t *d_out, uint32_t *d_out_read,
                          void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!params || (params->flags & ~kReportFlags)) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (!d_rep_off || (N && (!d_seeds || !d_seed_off || !d_off2 || !d_out || !d_tmp || tmp_bytes < scan_tmp_bytes(N)))) return RBG_EARG;
    return launch_report_select(reinterpret_cast<const uint64_t *>(d_seeds), d_seed_off, d_off2, N, d_first_fwd, params->read_len, params->min_seed_len,
                                params->flags, d_rep_off, d_out, d_out_read, d_tmp, tmp_bytes, stream) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_markers_report(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd, const rbg_report_params_t *params,
                       uint64_t *seed_off, rbg_report_seed_t **seeds, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!seed_off || !seeds || !mk) return RBG_EARG;
    *seeds = nullptr;
    *mk = nullptr;
    ReportOut o;
    o.seed_off = seed_off;
    seed_off[0] = 0;
    int rc = report_run(ix, seqs, off, N, first_fwd, params, o);
    if (rc) return rc;
    auto *h_recs = static_cast<rbg_report_seed_t *>(alloc_result(o.recs.size() * sizeof(rbg_report_seed_t)));
    auto *h_mk = static_cast<uint64_t *>(alloc_result(o.mk.size() * 8));
    if (!h_recs || !h_mk) { rbg_free_buffer(h_recs); rbg_free_buffer(h_mk); return RBG_ENOMEM; }
    if (!o.recs.empty()) std::memcpy(h_recs, o.recs.data(), o.recs.size() * sizeof(rbg_report_seed_t));
    if (!o.mk.empty()) std::memcpy(h_mk, o.mk.data(), o.mk.size() * 8);
    *seeds = h_recs;
    *mk = h_mk;
    return RBG_OK;
    });
}

int rbg_markers_tally(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd, const rbg_report_params_t *params,
                      rbg_tally *tally) {
    return guarded([&]() -> int {
    if (!tally || !ix || tally->ix->device != ix->device) return RBG_EARG;
    ReportOut o;
    o.tally = tally;
    return report_run(ix, seqs, off, N, first_fwd, params, o);
    });
}

int rbg_markers_report_text(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd, const rbg_report_params_t *params,
                            const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, const char **text, uint64_t *text_len) {
    return guarded([&]() -> int {
    if (!text || !text_len || (N && (!name_base || !name_begin || !name_len))) return RBG_EARG;
    *text = nullptr;
    *text_len = 0;
    ReportOut o;
    o.want_text = true;
    o.name_base = name_base;
    o.name_begin = name_begin;
    o.name_len = name_len;
    int rc = report_run(ix, seqs, off, N, first_fwd, params, o);
    if (rc) return rc;
    *text = o.text;
    *text_len = o.text_len;
    return RBG_OK;
    });
}

}  // extern "C"
