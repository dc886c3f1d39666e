// capi/report.ipp -- rb_markers' report on the device (k_report.hip): the device steps and the three host calls above them (records, text, tally), one
// pass of reads at a time: stage + strands, the seed pass (seeds.ipp), canon + select, then one of emit_records / emit_text / emit_tally.  Part of rbg_capi.hip.
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

// one pass's share of the trace: lap(slot) charges the time since the last lap to a slot.  Without tracing it does nothing, a synchronisation least of all.
struct ReportLap {
    hipStream_t st;
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point from = std::chrono::steady_clock::now();
    void operator()(int slot) {
        if (!g_report_trace.on) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        t[slot] += std::chrono::duration<double>(now - from).count();
        from = now;
    }
    void done(uint64_t reads, uint64_t d2h_bytes) {   // a finished pass joins the process's sums
        if (!g_report_trace.on) return;
        std::lock_guard<std::mutex> g(g_report_trace.mu);
        for (int j = 0; j < 8; ++j) g_report_trace.t[j] += t[j];
        g_report_trace.passes += 1;
        g_report_trace.reads += reads;
        g_report_trace.d2h += d2h_bytes;
    }
};

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
    uint32_t tally_flags = 0;   // RBG_TALLY_PER_READ [| RBG_TALLY_DROP_SITE_CONFLICTS]; 0: every line counts
};

struct ReportPass {   // reads [a, b) of the batch on the device, from step to step
    uint64_t a = 0, n = 0, bytes = 0;        // the first read, how many, their bytes
    uint64_t batch_bytes = 0;                // (of all N reads)
    bool last = false;
    ReportLap lap;
    uint64_t d2h_bytes = 0;
    DevBuf draw, doff, dcoin, dseq2, doff2;  // stage: the raw reads, their offsets and coins; the 2n strands and theirs
    std::vector<uint64_t> roff;              // (the offsets on the host: an asynchronous copy reads them, so they live as long as the pass)
    const uint8_t *d_coin = nullptr;
    SeedPass seeds;                          // the strands' seed records (canonical after select_records) and markers
    DevBuf dctmp, drep, drecs, dread, dstmp, dmelem, dws;   // select: printed records per read, the records, their reads; the element map of the outputs
    DevBuf dspan;                            // per-read tally: every record's read as a record range
    size_t stmp_bytes = 0, ws_bytes = 0;
    uint64_t R = 0, M = 0, E = 0;            // printed records, their markers, R + M
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

// the raw reads and their offsets go in (off[a] is not 0 in a later pass: the strand kernel subtracts it), the 2n strands come out
int stage_strands(const uint8_t *seqs, const uint64_t *off, const uint8_t *first_fwd, const rbg_report_params_t &P, ReportPass &p, hipStream_t st) {
    const uint64_t a = p.a, n = p.n, b = a + n;
    int rc;
    const uint64_t first16 = off[a] & ~uint64_t(15), raw_bytes = off[b] - first16;
    p.roff.resize(n + 1);
    for (uint64_t i = 0; i <= n; ++i) p.roff[i] = off[a + i] - first16;
    if ((rc = p.draw.alloc(((raw_bytes + 15) & ~uint64_t(15)) + 16)) || (rc = p.doff.alloc((n + 1) * 8)) ||
        (rc = p.dseq2.alloc(((2 * p.bytes + 15) & ~uint64_t(15)) + 16)) || (rc = p.doff2.alloc((2 * n + 1) * 8)))
        return rc;
    if (raw_bytes) HIP_TRY(hipMemcpyAsync(p.draw.p, seqs + first16, raw_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p.doff.p, p.roff.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    if (first_fwd && (P.flags & RBG_REPORT_HEURISTIC)) {
        if ((rc = p.dcoin.alloc(n))) return rc;
        HIP_TRY(hipMemcpyAsync(p.dcoin.p, first_fwd + a, n, hipMemcpyHostToDevice, st));
        p.d_coin = p.dcoin.as<uint8_t>();
    }
    return launch_read_strands(p.draw.as<uint8_t>(), p.doff.as<uint64_t>(), n, p.bytes, p.dseq2.as<uint8_t>(), p.doff2.as<uint64_t>(), st) ? RBG_ENODEV : RBG_OK;
}

// canonical records, then the printed records of every read: R of them in drecs, the read of each in dread
int select_records(rbg_index *ix, const rbg_report_params_t &P, ReportOut &o, ReportPass &p, hipStream_t st) {
    SeedPass &sp = p.seeds;
    const uint64_t n = p.n, S = sp.S;
    int rc;
    const size_t ctmp_bytes = seed_canon_tmp_bytes(S);
    if ((rc = p.dctmp.alloc(ctmp_bytes))) return rc;
    const uint32_t cflags = (P.flags & RBG_REPORT_HEURISTIC) ? P.flags & (RBG_REPORT_CLEAR_CONFLICTING | RBG_REPORT_CLEAR_IDENTICAL) : 0;
    if (sp.total_mk && launch_seed_canon(ix->cfg, sp.dseeds.as<uint64_t>(), S, sp.dmk.as<uint64_t>(), P.min_range, cflags, P.read_len, p.dctmp.p, ctmp_bytes, report_canon_group(), st))
        return RBG_ENODEV;
    p.lap(3);
    p.stmp_bytes = scan_tmp_bytes(std::max<uint64_t>(n, S));
    if ((rc = p.drep.alloc((n + 1) * 8)) || (rc = p.drecs.alloc(S * sizeof(rbg_report_seed_t))) || (rc = p.dread.alloc(S * 4)) || (rc = p.dstmp.alloc(p.stmp_bytes)) ||
        (rc = p.dmelem.alloc((S + 1) * 8)))
        return rc;
    if (launch_report_select(sp.dseeds.as<uint64_t>(), sp.d_rec_off, p.doff2.as<uint64_t>(), n, p.d_coin, P.read_len, P.min_seed_len, P.flags, p.drep.as<uint64_t>(), p.drecs.p,
                             p.dread.as<uint32_t>(), p.dstmp.p, p.stmp_bytes, st))
        return RBG_ENODEV;
    if (o.want_text || o.tally) {   // (only the records output tells its caller which read printed what)
        HIP_TRY(hipMemcpyAsync(&p.R, p.drep.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return RBG_OK;
    }
    std::vector<uint64_t> rep_off(n + 1);
    HIP_TRY(hipMemcpyAsync(rep_off.data(), p.drep.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    p.R = rep_off[n];
    const uint64_t base = o.recs.size();
    for (uint64_t i = 0; i < n; ++i) o.seed_off[p.a + i + 1] = base + rep_off[i + 1];
    return RBG_OK;
}

// records: the printed records and their markers, dense, behind what the passes before left in o
int emit_records(ReportOut &o, ReportPass &p, hipStream_t st) {
    const uint64_t R = p.R, M = p.M;
    int rc;
    DevBuf drecs2, ddense;
    if ((rc = drecs2.alloc(R * sizeof(rbg_report_seed_t))) || (rc = ddense.alloc(M * 8))) return rc;
    if (launch_report_gather(p.drecs.p, p.dmelem.as<uint64_t>(), p.seeds.dmk.as<uint64_t>(), R, p.E, p.dws.p, p.ws_bytes, drecs2.p, ddense.as<uint64_t>(), st)) return RBG_ENODEV;
    p.lap(5);
    const uint64_t rbase = o.recs.size(), mbase = o.mk.size();
    o.recs.resize(rbase + R);
    o.mk.resize(mbase + M);
    if ((rc = d2h_result(o.recs.data() + rbase, drecs2.p, R * sizeof(rbg_report_seed_t), st))) return rc;
    if (M && (rc = d2h_result(o.mk.data() + mbase, ddense.p, M * 8, st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    rebase_markers(o.recs.data() + rbase, R, mbase);
    p.d2h_bytes = R * sizeof(rbg_report_seed_t) + M * 8 + (p.n + 1) * 8;
    return RBG_OK;
}

// a pass's text to its place in the call's pinned buffer.  behind: the last pass's copy runs on the handle's copy stream behind the fill kernel; the caller
// returns at once and the text's reader waits (rbg_wait_text), as in rbg_align_text
int copy_text_out(rbg_index *ix, ReportOut &o, char *dst, DevBuf &dtext, uint64_t total, bool behind, hipStream_t st) {
    if (!behind) {
        HIP_TRY(hipMemcpyAsync(dst, dtext.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return RBG_OK;
    }
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
    return RBG_OK;
}

// text: the pass's lines written on the device, copied behind the text of the passes before
int emit_text(rbg_index *ix, ReportOut &o, ReportPass &p, hipStream_t st) {
    const uint64_t a = p.a, n = p.n, R = p.R, E = p.E;
    int rc;
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
    if (launch_report_text_plan(p.drecs.p, p.dread.as<uint32_t>(), p.dmelem.as<uint64_t>(), p.seeds.dmk.as<uint64_t>(), R, E, dnames.as<char>(), dnoff.as<uint32_t>(), p.dws.p,
                                p.ws_bytes, st))
        return RBG_ENODEV;
    const uint64_t *p_at = nullptr;
    const uint32_t *p_len = nullptr;
    report_text_total_ptrs(p.dws.p, E, &p_at, &p_len);
    uint64_t last_at = 0;
    uint32_t last_len = 0;
    HIP_TRY(hipMemcpyAsync(&last_at, p_at, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_len, p_len, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the name blob has been copied too)
    const uint64_t total = last_at + last_len;
    if ((rc = dtext.alloc(total))) return rc;
    if (launch_report_text_fill(p.drecs.p, p.dread.as<uint32_t>(), p.dmelem.as<uint64_t>(), p.seeds.dmk.as<uint64_t>(), R, E, dnames.as<char>(), dnoff.as<uint32_t>(), p.dws.p,
                                p.ws_bytes, total, dtext.as<char>(), st))
        return RBG_ENODEV;
    p.lap(5);
    // (a first pass that is not the last sizes the buffer for the whole batch from its own text per read byte)
    const size_t hint = p.last || !p.bytes ? 0 : static_cast<size_t>(static_cast<double>(total) / static_cast<double>(p.bytes) * static_cast<double>(p.batch_bytes) * 1.25);
    if ((rc = report_text_room(ix, o, o.text_len + total, hint))) return rc;
    char *dst = o.text + o.text_len;
    o.text_len += total;
    p.d2h_bytes = total;
    return copy_text_out(ix, o, dst, dtext, total, p.last && !g_report_trace.on, st);
}

// tally: room was reserved between the seed phases; the add is the pass's last launch and nothing comes back
int emit_tally(ReportOut &o, ReportPass &p, hipStream_t st) {
    if (!o.tally_flags) return tally_add_mapped(o.tally, p.drecs.p, p.R, p.seeds.dmk.as<uint64_t>(), p.dmelem.as<uint64_t>(), p.seeds.total_mk, st);
    int rc = p.dspan.alloc(tally_span_bytes(p.R));   // per-read mode: drep tells which records are one read's (a pass holds whole reads)
    if (rc) return rc;
    return tally_add_mapped(o.tally, p.drecs.p, p.R, p.seeds.dmk.as<uint64_t>(), p.dmelem.as<uint64_t>(), p.seeds.total_mk, st, o.tally_flags, p.drep.as<uint64_t>(), p.n,
                            p.dspan.p);
}

// reads [a, b) of the batch: strands -> seeds -> canon -> select -> records, text or tally.  The trace's slots in their order: 0 copy in + strands, 1 plan,
// 2 fill, 3 canon (select_records laps it before its second launch), 4 select, then 7 tally, or 5 gather or text (the emit laps it before it copies) and 6 copy out
int report_pass(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t a, uint64_t b, uint64_t N, const uint8_t *first_fwd,
                const rbg_report_params_t &P, ReportOut &o, hipStream_t st) {
    ReportPass p;
    p.a = a; p.n = b - a; p.bytes = off[b] - off[a]; p.batch_bytes = off[N] - off[0]; p.last = b == N;
    p.lap.st = st;
    SeedPass &sp = p.seeds;
    const bool lmem = (P.flags & RBG_REPORT_LMEM) != 0;
    int rc;
    if ((rc = stage_strands(seqs, off, first_fwd, P, p, st))) return rc;
    p.lap(0);
    if (lmem && p.bytes >> 31) return RBG_EARG;   // (lmem: S = 2 * bytes is known before the plan, which sizes its scratch by it)
    if ((rc = seed_pass_plan(ix, sp, p.dseq2.as<uint8_t>(), p.doff2.as<uint64_t>(), 2 * p.n, 2 * p.bytes, P.wsize, P.max_range, P.ftab_k, lmem, st))) return rc;
    p.lap(1);
    if (sp.S >> 32) return RBG_EARG;   // (a pass holds at most 64 MiB of reads)
    if (o.tally && (rc = tally_reserve(o.tally, sp.total_mk))) return rc;   // (total_mk bounds the pass's elements from above: canon and select only drop)
    if ((rc = seed_pass_fill(ix, sp, st))) return rc;
    p.lap(2);
    if ((rc = select_records(ix, P, o, p, st))) return rc;
    p.lap(4);
    if (p.R) {
        if (launch_report_melem(p.drecs.p, p.R, p.dmelem.as<uint64_t>(), p.dstmp.p, p.stmp_bytes, st)) return RBG_ENODEV;
        if (o.tally) {
            if ((rc = emit_tally(o, p, st))) return rc;
            p.lap(7);
        } else {   // the element -> record map of the printed records' markers, for the records and the text (the tally keeps a map of its own)
            HIP_TRY(hipMemcpyAsync(&p.M, p.dmelem.as<uint64_t>() + p.R, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            p.E = p.R + p.M;
            p.ws_bytes = report_text_ws_bytes(p.E);
            if ((rc = p.dws.alloc(p.ws_bytes))) return rc;
            if (launch_report_map(p.dmelem.as<uint64_t>(), p.R, p.E, p.dws.p, p.ws_bytes, st)) return RBG_ENODEV;
            if ((rc = o.want_text ? emit_text(ix, o, p, st) : emit_records(o, p, st))) return rc;
            p.lap(6);
        }
    } else if (o.tally && (o.tally_flags & RBG_TALLY_PER_READ)) {
        o.tally->reads += p.n;   // (reads seen, though none of them printed a line)
    }
    p.lap.done(p.n, p.d2h_bytes);
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
        const uint64_t b = pass_end(off, N, a, chunk, uint64_t(1) << 28);   // (2^31 records' worth of reads at most)
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

int rbg_markers_tally_reads(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, const uint8_t *first_fwd, const rbg_report_params_t *params,
                            uint32_t tally_flags, rbg_tally *tally) {
    return guarded([&]() -> int {
    if (!tally || !ix || tally->ix->device != ix->device || !tally_flags_ok(tally_flags)) return RBG_EARG;
    ReportOut o;
    o.tally = tally;
    o.tally_flags = tally_flags;
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
