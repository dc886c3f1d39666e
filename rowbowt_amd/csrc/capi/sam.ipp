// capi/sam.ipp -- rbg_align_sam (SAM lines of a batch of raw reads, both strands, made on the device: k_sam.hip), rbg_align_sam_extend (the same call with
// every line's seed extended leftwards through mismatches by an LF walk: sam_extend.hip), rbg_extend_left_dev (that walk alone) and rbg_sam_header (host).  Part of
// rbg_capi.hip.  The steps: the call's inputs through one pinned block (launch_copy16), k_sam_strands, launch_greedy_seed over the 2N sequences, k_sam_pick,
// the locate plan / order / fill of seeds.ipp over the picked ranges, then k_sam.hip's plan and fill; the text leaves through the handle's pinned text
// buffers as rbg_align_text's does (text.ipp).  The extended call runs the same steps through the locate fill, then sam_extend.hip's: every line's read,
// document and walk item, k_extend_left over the lines, the extended lengths, k_sam.hip's offsets, the extended text.  rbg_align_sam_extend_both adds, behind
// the left walks, fl_extend.hip's right items and k_extend_right over the lines with a right clip (the handle's FL index: capi/fl.ipp), and takes the lengths
// and the text from the kernels that format both records.
namespace {
// RBG_SAM_TRACE=1: where rbg_align_sam spends its time (each step synchronised), summed over the process's calls and printed at exit
struct SamTrace {
    const char *what;
    bool extend;       // the extended call: one more column, the lines' LF walks
    bool right = false;   // rbg_align_sam_extend_both: a further column, the lines' FL walks
    bool on = std::getenv("RBG_SAM_TRACE") != nullptr;
    std::mutex mu;
    double t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t calls = 0, bytes = 0;
    // the extended call, from the lines' records: lines, lines with a clipped prefix (a > 0: the walks), bases taken, mismatches taken, lines extended at
    // all, extended bases, lines whose left clip went to zero
    uint64_t walks[7] = {0, 0, 0, 0, 0, 0, 0};
    // the call extended on both sides, from the right records: lines with a right clip, lines walked (an item), FL steps that cross seeds, FL steps compared,
    // mismatches taken, lines extended at all, extended bases, right clips gone
    uint64_t rwalks[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    SamTrace(const char *w, bool x, bool r = false) : what(w), extend(x), right(r) {}
    ~SamTrace() {
        if (!(on && calls)) return;
        std::fprintf(stderr, "%s: %llu calls, %.1f MB of text: copy in %.3f s, strands %.3f, search %.3f, pick %.3f, locate %.3f, ", what,
                     static_cast<unsigned long long>(calls), static_cast<double>(bytes) / 1e6, t[0], t[1], t[2], t[3], t[4]);
        if (extend) std::fprintf(stderr, "extend %.3f, ", t[8]);
        if (right) std::fprintf(stderr, "extend right %.3f, ", t[9]);
        std::fprintf(stderr, "text plan %.3f, text fill %.3f, copy out %.3f\n", t[5], t[6], t[7]);
        if (extend)
            std::fprintf(stderr, "%s walks: %llu lines, %llu with a clipped prefix, %llu LF steps, %llu of them mismatches taken (the others hit at the first "
                                 "request), %llu lines extended by %llu bases, %llu left clips gone\n", what, static_cast<unsigned long long>(walks[0]),
                         static_cast<unsigned long long>(walks[1]), static_cast<unsigned long long>(walks[2]), static_cast<unsigned long long>(walks[3]),
                         static_cast<unsigned long long>(walks[4]), static_cast<unsigned long long>(walks[5]), static_cast<unsigned long long>(walks[6]));
        if (right)
            std::fprintf(stderr, "%s right walks: %llu lines, %llu walked (a right clip inside the document), %llu FL steps across seeds, %llu FL steps compared, %llu of them "
                                 "mismatches taken, %llu lines extended by %llu bases, %llu right clips gone\n", what, static_cast<unsigned long long>(rwalks[0]),
                         static_cast<unsigned long long>(rwalks[1]), static_cast<unsigned long long>(rwalks[2]), static_cast<unsigned long long>(rwalks[3]),
                         static_cast<unsigned long long>(rwalks[4]), static_cast<unsigned long long>(rwalks[5]), static_cast<unsigned long long>(rwalks[6]),
                         static_cast<unsigned long long>(rwalks[7]));
    }
};
SamTrace g_sam_trace("rbg_align_sam", false), g_sam_ext_trace("rbg_align_sam_extend", true), g_sam_both_trace("rbg_align_sam_extend_both", true, true);
static_assert(sizeof(rbg_extend_t) == sizeof(SamExtend) && offsetof(rbg_extend_t, mis_t) == offsetof(SamExtend, mis_t) &&
              offsetof(rbg_extend_t, mis_ref) == offsetof(SamExtend, mis_ref) && RBG_SAM_MAX_MISMATCH == 8, "rbg.h mirrors rbg_sam.hpp");

// max_mismatch < 0: rbg_align_sam's lines; else the extended lines with that budget, `right`: on both sides (the handle's FL index must be prepared)
int align_sam_lines(rbg_index *ix, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len, const char *qual_base, const uint64_t *qual_begin,
                    const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N, uint64_t min_length, uint64_t max_hits,
                    uint32_t flags, int max_mismatch, bool right, const char **text, uint64_t *text_len) {
    const bool extend = max_mismatch >= 0;
    SamTrace &g_trace = right ? g_sam_both_trace : extend ? g_sam_ext_trace : g_sam_trace;
    if (!queryable(ix)) return RBG_ENODEV;
    if (right && !fl_ready(ix)) return RBG_ENOTLOADED;
    if (flags & ~static_cast<uint32_t>(RBG_SAM_SECONDARY)) return RBG_EARG;
    if (!ix->H().has_tsa || !ix->H().has_dl) return RBG_ENOTLOADED;
    if (min_length == 0) return RBG_EARG;   // (a zero-length seed has the full range)
    if (!text || !text_len || (N >> 32) || (N && (!seq_base || !seq_begin || !seq_len || !name_base || !name_begin || !name_len || (qual_base && !qual_begin))))
        return RBG_EARG;
    *text = nullptr;
    *text_len = 0;
    if (N == 0) return RBG_OK;
    const uint64_t walk_hits = (flags & RBG_SAM_SECONDARY) ? std::max<uint64_t>(max_hits, 1) : 1;   // (the primary line is always there)
    uint64_t seq_bytes = 0, name_bytes = 0;   // (argument errors are answered before anything touches the device)
    for (uint64_t i = 0; i < N; ++i) { seq_bytes += seq_len[i]; name_bytes += name_len[i]; }
    if ((seq_bytes >> 32) || (name_bytes >> 32)) return RBG_EARG;
    // RBG_SAM_GRID_CAP=<workgroups>: a test-and-A/B switch, read once per call (set it before the call, not during one)
    const uint32_t cap = [] { const char *e = std::getenv("RBG_SAM_GRID_CAP"); const long long v = e && *e ? std::atoll(e) : 0;
                              return v > 0 && v < (1ll << 31) ? static_cast<uint32_t>(v) : 0u; }();
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    int rc = ensure_text_docs(ix);
    if (rc) return rc;
    hipStream_t st = hipStreamPerThread;
    double lap_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto lap_from = std::chrono::steady_clock::now();
    auto lap = [&](int slot) {
        if (!g_trace.on) return;
        (void)hipStreamSynchronize(st);
        const auto now = std::chrono::steady_clock::now();
        lap_t[slot] += std::chrono::duration<double>(now - lap_from).count();
        lap_from = now;
    };
    // ONE pinned block: [read offsets u64 | name offsets u32 | reads | qualities | names], the byte areas 16-byte aligned
    auto up16 = [](size_t x) { return (x + 15) & ~size_t(15); };
    const size_t o_roff = 0, o_noff = (N + 1) * 8, o_seq = up16(o_noff + (N + 1) * 4), o_qual = o_seq + up16(seq_bytes) + 16,
                 o_names = o_qual + (qual_base ? up16(seq_bytes) + 16 : 0), in_bytes = o_names + up16(name_bytes) + 16;
    TextInHold in(ix);
    if ((rc = in.take(in_bytes))) return rc;
    uint64_t *roff = reinterpret_cast<uint64_t *>(in.p + o_roff);
    uint32_t *noff = reinterpret_cast<uint32_t *>(in.p + o_noff);
    {
        uint64_t racc = 0;
        uint32_t nacc = 0;
        for (uint64_t i = 0; i < N; ++i) { roff[i] = racc; racc += seq_len[i]; noff[i] = nacc; nacc += name_len[i]; }
        roff[N] = racc;
        noff[N] = nacc;
    }
    parallel_for(N, [&](uint64_t a, uint64_t b, unsigned) {
        for (uint64_t i = a; i < b; ++i) {
            std::memcpy(in.p + o_seq + roff[i], seq_base + seq_begin[i], seq_len[i]);
            if (qual_base) std::memcpy(in.p + o_qual + roff[i], qual_base + qual_begin[i], seq_len[i]);
            std::memcpy(in.p + o_names + noff[i], name_base + name_begin[i], name_len[i]);
        }
    });
    DevBuf din, dseq2, doff2, dseed, dpick, drev, dlines, dloff, dtmp, dbad;
    const size_t tmp_bytes = std::max(scan_tmp_bytes(N), sam_pick_tmp_bytes(N));
    if ((rc = din.alloc(in_bytes)) || (rc = dseq2.alloc(up16(2 * seq_bytes) + 16)) || (rc = doff2.alloc((2 * N + 1) * 8)) || (rc = dseed.alloc(5 * 2 * N * 8)) ||
        (rc = dpick.alloc(5 * N * 8)) || (rc = drev.alloc(N)) || (rc = dlines.alloc(2 * (N + 1) * 8)) || (rc = dloff.alloc((N + 1) * 8)) ||
        (rc = dtmp.alloc(tmp_bytes)) || (rc = dbad.alloc(16)))
        return rc;
    // the copy kernel reads the pinned block, which goes back to its pool when this call returns: an error return below waits for the stream first
    // (the success path has waited by then: the locate plan's read-back)
    struct DrainOnExit { hipStream_t st; bool armed; ~DrainOnExit() { if (armed) (void)hipStreamSynchronize(st); } } drain{st, true};
    if (launch_copy16(in.p, din.p, in_bytes - 16, st)) return RBG_ENODEV;
    HIP_TRY(hipMemsetAsync(dbad.p, 0, 16, st));
    const uint64_t *d_roff = reinterpret_cast<const uint64_t *>(din.as<char>() + o_roff);
    const uint32_t *d_noff = reinterpret_cast<const uint32_t *>(din.as<char>() + o_noff);
    const char *d_seq = din.as<char>() + o_seq, *d_qual = qual_base ? din.as<char>() + o_qual : nullptr, *d_names = din.as<char>() + o_names;
    lap(0);
    if (launch_sam_strands(reinterpret_cast<const uint8_t *>(d_seq), d_roff, N, seq_bytes, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), cap, st)) return RBG_ENODEV;
    lap(1);
    uint64_t *s_lo = dseed.as<uint64_t>(), *s_hi = s_lo + 2 * N, *s_qs = s_hi + 2 * N, *s_qe = s_qs + 2 * N, *s_ss = s_qe + 2 * N;
    if (launch_greedy_seed(ix->dev, ix->cfg, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), 2 * N, min_length, s_lo, s_hi, s_qs, s_qe, s_ss, st)) return RBG_ENODEV;
    lap(2);
    uint64_t *p_lo = dpick.as<uint64_t>(), *p_hi = p_lo + N, *p_k = p_hi + N, *p_a = p_k + N, *p_b = p_a + N;
    uint64_t *nlines = dlines.as<uint64_t>(), *line_off = nlines + (N + 1);
    if (launch_sam_pick(s_lo, s_hi, s_qs, s_qe, s_ss, N, walk_hits, p_lo, p_hi, p_k, p_a, p_b, drev.as<uint8_t>(), nlines, line_off, ix->dev.counters, dtmp.p,
                        tmp_bytes, cap, st))
        return RBG_ENODEV;
    lap(3);
    // locs_at over the picked ranges, as greedy_host does it (seeds.ipp): the locations never leave the device
    uint64_t nlocs = 0, E = 0;
    if (launch_locate_plan(ix->dev, ix->cfg, p_lo, p_hi, N, walk_hits, dloff.as<uint64_t>(), dtmp.p, tmp_bytes, st)) return RBG_ENODEV;
    HIP_TRY(hipMemcpyAsync(&nlocs, dloff.as<uint64_t>() + N, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&E, line_off + N, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    drain.armed = false;
    DevBuf dlocs, dord, dws, dtext;
    if ((rc = dlocs.alloc(nlocs * 8))) return rc;
    const void *order = nullptr;
    if ((rc = make_order(ix, p_k, N, dord, st, &order))) return rc;
    if (nlocs && launch_locate_fill(ix->dev, ix->cfg, p_lo, p_hi, p_k, N, walk_hits, dloff.as<uint64_t>(), dlocs.as<uint64_t>(), nullptr, order, st)) return RBG_ENODEV;
    lap(4);
    const size_t ws_bytes = sam_ws_bytes(E);
    if ((rc = dws.alloc(ws_bytes))) return rc;
    const auto &D = ix->text_docs;
    const SamBatch B{N, E, p_lo, p_hi, p_a, p_b, drev.as<uint8_t>(), line_off, dloff.as<uint64_t>(), dlocs.as<uint64_t>(), d_seq, d_qual, d_roff, d_names, d_noff,
                     D.start, D.names, D.name_off, D.n, D.size};
    DevBuf ditem, dext, dritem, drext;
    if (extend) {
        // per line 24 bytes of item {row, limit, sequence, a} and the 56-byte record; the second word of dbad is the walk's error word (never set here:
        // the items come from the call's own arrays)
        if ((rc = ditem.alloc(E * 24)) || (rc = dext.alloc(E * sizeof(SamExtend)))) return rc;
        uint64_t *i_row = ditem.as<uint64_t>(), *i_lim = i_row + E;
        uint32_t *i_seq = reinterpret_cast<uint32_t *>(i_lim + E), *i_a = i_seq + E;
        if (launch_sam_ext_items(B, dws.p, i_seq, i_a, i_row, i_lim, dbad.as<unsigned int>(), cap, st)) return RBG_ENODEV;
        if (launch_extend_left(ix->dev, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), 2 * N, i_seq, i_a, i_row, i_lim, E, static_cast<uint32_t>(max_mismatch), dext.p,
                               dbad.as<unsigned int>() + 1, cap, st))
            return RBG_ENODEV;
        lap(8);
        if (g_trace.on) {   // the records' sums, outside every column (the clock starts again once the host copies are gone)
            {
            std::vector<SamExtend> hx(E);
            std::vector<uint32_t> ha(E);
            HIP_TRY(hipMemcpyAsync(hx.data(), dext.p, E * sizeof(SamExtend), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ha.data(), i_a, E * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            uint64_t w[7] = {E, 0, 0, 0, 0, 0, 0};
            for (uint64_t e = 0; e < E; ++e) {
                w[1] += ha[e] > 0;
                w[2] += hx[e].steps;
                for (int j = 0; j < RBG_SAM_MAX_MISMATCH; ++j) w[3] += hx[e].mis_ref[j] != 0;
                w[4] += hx[e].ext > 0;
                w[5] += hx[e].ext;
                w[6] += ha[e] > 0 && hx[e].ext == ha[e];
            }
            std::lock_guard<std::mutex> g(g_trace.mu);
            for (int j = 0; j < 7; ++j) g_trace.walks[j] += w[j];
            }
            lap_from = std::chrono::steady_clock::now();
        }
        if (right) {
            // per line 32 bytes of item {row, limit, sequence, b, skip, budget} and the right record; the third word of dbad is this walk's error word
            if ((rc = dritem.alloc(E * 32)) || (rc = drext.alloc(E * sizeof(SamExtend)))) return rc;
            uint64_t *r_row = dritem.as<uint64_t>(), *r_lim = r_row + E;
            uint32_t *r_seq = reinterpret_cast<uint32_t *>(r_lim + E), *r_b = r_seq + E, *r_skip = r_b + E, *r_k = r_skip + E;
            if (launch_sam_right_items(B, dws.p, dext.p, ix->H().n, static_cast<uint32_t>(max_mismatch), r_seq, r_b, r_row, r_skip, r_lim, r_k, cap, st)) return RBG_ENODEV;
            if (launch_extend_right(ix->fl_dev.view, ix->H().pos_bytes, ix->H().n, dseq2.as<uint8_t>(), doff2.as<uint64_t>(), 2 * N, r_seq, r_b, r_row, r_skip, r_lim, r_k,
                                    E, static_cast<uint32_t>(max_mismatch), drext.p, dbad.as<unsigned int>() + 2, cap, st))
                return RBG_ENODEV;
            lap(9);
            if (g_trace.on) {
                {
                std::vector<SamExtend> hx(E);
                std::vector<uint32_t> hs(E), hb(E), hk(E);
                HIP_TRY(hipMemcpyAsync(hx.data(), drext.p, E * sizeof(SamExtend), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(hs.data(), r_seq, E * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(hb.data(), r_b, E * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(hk.data(), r_skip, E * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                uint64_t w[8] = {E, 0, 0, 0, 0, 0, 0, 0};
                for (uint64_t e = 0; e < E; ++e) {
                    if (hs[e] == 0xFFFFFFFFu) continue;
                    const uint64_t clip = seq_len[hs[e] >> 1] - hb[e];
                    w[1] += 1;
                    w[2] += hk[e];
                    w[3] += hx[e].steps;
                    for (int j = 0; j < RBG_SAM_MAX_MISMATCH; ++j) w[4] += hx[e].mis_ref[j] != 0;
                    w[5] += hx[e].ext > 0;
                    w[6] += hx[e].ext;
                    w[7] += hx[e].ext == clip;
                }
                std::lock_guard<std::mutex> g(g_trace.mu);
                for (int j = 0; j < 8; ++j) g_trace.rwalks[j] += w[j];
                }
                lap_from = std::chrono::steady_clock::now();
            }
        }
        if ((right ? launch_sam_both_len(B, dws.p, dext.p, drext.p, cap, st) : launch_sam_ext_len(B, dws.p, dext.p, cap, st)) || launch_sam_offsets(dws.p, E, st))
            return RBG_ENODEV;
    } else if (launch_sam_plan(B, dws.p, ws_bytes, dbad.as<unsigned int>(), cap, st)) {
        return RBG_ENODEV;
    }
    const uint64_t *p_at = nullptr, *p_len = nullptr;
    sam_total_ptrs(dws.p, E, &p_at, &p_len);
    uint64_t last_at = 0, last_len = 0;
    uint32_t bad[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&last_at, p_at, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&last_len, p_len, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(bad, dbad.p, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap(5);
    if (extend && (bad[1] || bad[2])) return RBG_ENODEV;   // (an item of the call's own making refused by a walk: cannot happen)
    if (bad[0]) return RBG_EARG;   // a location before every document: rbg_resolve_offset's error, as rbg_align_text answers
    const uint64_t total = last_at + last_len;
    if ((rc = dtext.alloc(total))) return rc;
    if (right    ? launch_sam_both_fill(B, dws.p, dext.p, drext.p, total, dtext.as<char>(), cap, st)
        : extend ? launch_sam_ext_fill(B, dws.p, dext.p, total, dtext.as<char>(), cap, st)
                 : launch_sam_fill(B, dws.p, total, dtext.as<char>(), cap, st))
        return RBG_ENODEV;
    lap(6);
    char *out = nullptr;
    if ((rc = take_text_out(ix, total, &out))) return rc;
    {   // the copy-out on the handle's copy stream, behind the fill kernel: rbg_align_text's protocol (rbg_wait_text / rbg_release_text)
        std::lock_guard<std::mutex> g(ix->text_mu);
        rbg_index::TextOut *t = find_text_out(ix, out);
        hipError_t e = hipEventRecord(t->done, st);
        if (e == hipSuccess) e = hipStreamWaitEvent(ix->text_copy_stream, t->done, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(out, dtext.p, total, hipMemcpyDeviceToHost, ix->text_copy_stream);
        if (e == hipSuccess) e = hipEventRecord(t->done, ix->text_copy_stream);
        if (e != hipSuccess) { t->busy = false; HIP_TRY(e); }
        t->pending = true;
        t->d_text = dtext.p; t->d_cls = dtext.cls; t->d_dev = dtext.dev;
        dtext.p = nullptr;   // (the record owns the device block until the copy has been waited for)
    }
    if (g_trace.on) {
        (void)rbg_wait_text(ix, out);
        lap(7);
        std::lock_guard<std::mutex> g(g_trace.mu);
        for (int j = 0; j < 10; ++j) g_trace.t[j] += lap_t[j];
        g_trace.calls += 1;
        g_trace.bytes += total;
    }
    *text = out;
    *text_len = total;
    return RBG_OK;
}
}  // namespace
extern "C" {

int rbg_align_sam(rbg_index *ix, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len, const char *qual_base, const uint64_t *qual_begin,
                  const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N, uint64_t min_length, uint64_t max_hits,
                  uint32_t flags, const char **text, uint64_t *text_len) {
    return guarded([&]() -> int {
        return align_sam_lines(ix, seq_base, seq_begin, seq_len, qual_base, qual_begin, name_base, name_begin, name_len, N, min_length, max_hits, flags, -1, false, text,
                               text_len);
    });
}

int rbg_align_sam_extend(rbg_index *ix, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len, const char *qual_base, const uint64_t *qual_begin,
                         const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N, uint64_t min_length, uint64_t max_hits,
                         uint32_t flags, uint32_t max_mismatch, const char **text, uint64_t *text_len) {
    return guarded([&]() -> int {
        if (!ix || max_mismatch > RBG_SAM_MAX_MISMATCH) return RBG_EARG;   // (a null handle is an argument error here; a handle without a device: RBG_ENODEV)
        return align_sam_lines(ix, seq_base, seq_begin, seq_len, qual_base, qual_begin, name_base, name_begin, name_len, N, min_length, max_hits, flags,
                               static_cast<int>(max_mismatch), false, text, text_len);
    });
}

int rbg_align_sam_extend_both(rbg_index *ix, const char *seq_base, const uint64_t *seq_begin, const uint32_t *seq_len, const char *qual_base,
                              const uint64_t *qual_begin, const char *name_base, const uint64_t *name_begin, const uint32_t *name_len, uint64_t N,
                              uint64_t min_length, uint64_t max_hits, uint32_t flags, uint32_t max_mismatch, const char **text, uint64_t *text_len) {
    return guarded([&]() -> int {
        if (!ix || max_mismatch > RBG_SAM_MAX_MISMATCH) return RBG_EARG;
        return align_sam_lines(ix, seq_base, seq_begin, seq_len, qual_base, qual_begin, name_base, name_begin, name_len, N, min_length, max_hits, flags,
                               static_cast<int>(max_mismatch), true, text, text_len);
    });
}

int rbg_extend_left_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, const uint32_t *d_item_seq, const uint32_t *d_item_a,
                        const uint64_t *d_item_row, const uint64_t *d_item_limit, uint64_t M, uint32_t max_mismatch, rbg_extend_t *d_out, void *stream) {
    return guarded([&]() -> int {
    if (!ix || max_mismatch > RBG_SAM_MAX_MISMATCH) return RBG_EARG;
    if (!queryable(ix)) return RBG_ENODEV;
    if (M && (!d_seqs || !d_off || !d_item_seq || !d_item_a || !d_item_row || !d_item_limit || !d_out)) return RBG_EARG;
    if ((reinterpret_cast<uintptr_t>(d_seqs) & 15) || (reinterpret_cast<uintptr_t>(d_out) & 3)) return RBG_EARG;   // reads are fetched as aligned 16-byte chunks
    if (M == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    const uint32_t cap = [] { const char *e = std::getenv("RBG_SAM_GRID_CAP"); const long long v = e && *e ? std::atoll(e) : 0;
                              return v > 0 && v < (1ll << 31) ? static_cast<uint32_t>(v) : 0u; }();
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf derr;   // (released after the wait below: nothing of this call still runs on it)
    int rc = derr.alloc(16);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(derr.p, 0, 16, st));
    if (launch_extend_left(ix->dev, d_seqs, d_off, N, d_item_seq, d_item_a, d_item_row, d_item_limit, M, max_mismatch, d_out, derr.as<unsigned int>(), cap, st))
        return RBG_ENODEV;
    uint32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, derr.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return err ? RBG_EARG : RBG_OK;
    });
}

int rbg_sam_header(rbg_index *ix, const char *pg_line, char **text, uint64_t *text_len) {
    return guarded([&]() -> int {
    if (!ix || !text || !text_len) return RBG_EARG;
    *text = nullptr;
    *text_len = 0;
    const RawDocs &d = ix->H().dl;
    if (!ix->H().has_dl || d.names.empty() || d.sorted.size() != d.names.size()) return RBG_ENOTLOADED;
    const std::string s = sam_header_text(d.names, d.sorted, ix->H().n, pg_line);
    char *p = static_cast<char *>(alloc_result(s.size() + 1));
    if (!p) return RBG_ENOMEM;
    std::memcpy(p, s.c_str(), s.size() + 1);
    *text = p;
    *text_len = s.size();
    return RBG_OK;
    });
}

}  // extern "C"
