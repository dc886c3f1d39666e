// capi/seeds.ipp -- markers, marker seeds and greedy seeding (rb_markers' path), device and host entry points; the seed pass and the pass splitter
// that the host calls here and the report (report.ipp) share.  Part of rbg_capi.hip.
namespace {
// One device pass of marker seeds over n staged sequences, greedy (get_markers_greedy_seeding) or lmem (get_markers_lmems), in the kernels' two phases:
// seed_pass_plan() counts, seed_pass_fill() writes.  marker_seeds_host(), rbg_get_markers_lmems() and the report's report_pass() run their seeds
// through these two; what differs between them -- staging, copy-out, the tally's reserve between the phases -- stays with them.
struct SeedPass {
    DevBuf dsoff, dmoff, dtmp, dlog, dseeds, dmk;   // seed offsets and the log (greedy), marker offsets, scan scratch (lmem: the records' marker offsets too), records, markers
    size_t tmp_bytes = 0, log_bytes = 0;            // (log_bytes == 0: no log, the fill walks again)
    const uint8_t *d_seqs = nullptr;                // the plan's arguments, kept for the fill
    const uint64_t *d_off = nullptr;
    uint64_t n = 0, wsize = 0, max_range = 0, ftab_k = 0;
    bool lmem = false;
    uint64_t S = 0, total_mk = 0;                   // what the plan found: records and markers of the pass (lmem: one record per end position, S = the sequences' bytes)
    const uint64_t *d_rec_off = nullptr;            // on the device: the first record of every sequence, n + 1 values (greedy: the scanned dsoff; lmem: the sequences' own offsets)
};

// The n sequences are on the device, d_off[0] == 0 and d_off[n] == total_bytes.  Returns with the stream synchronised and S and total_mk known.
// h_seed_off (greedy, nullable): every sequence's first record for the caller, n + 1 values, out of the same copy-back.
int seed_pass_plan(rbg_index *ix, SeedPass &sp, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t n, uint64_t total_bytes, uint64_t wsize, uint64_t max_range,
                   uint64_t ftab_k, bool lmem, hipStream_t st, uint64_t *h_seed_off = nullptr) {
    sp.d_seqs = d_seqs; sp.d_off = d_off; sp.n = n; sp.wsize = wsize; sp.max_range = max_range; sp.ftab_k = ftab_k; sp.lmem = lmem;
    int rc;
    if (lmem) {
        sp.S = total_bytes;
        sp.d_rec_off = d_off;
        sp.tmp_bytes = marker_lmems_tmp_bytes(sp.S);
        if ((rc = sp.dmoff.alloc((n + 1) * 8)) || (rc = sp.dtmp.alloc(sp.tmp_bytes))) return rc;
        if (launch_marker_lmems_plan(ix->dev, ix->cfg, d_seqs, d_off, n, sp.S, wsize, max_range, ftab_k, sp.dmoff.as<uint64_t>(), sp.dtmp.p, sp.tmp_bytes, st)) return RBG_ENODEV;
    } else {
        sp.tmp_bytes = scan_tmp_bytes(n);
        if ((rc = sp.dsoff.alloc((n + 1) * 8)) || (rc = sp.dmoff.alloc((n + 1) * 8)) || (rc = sp.dtmp.alloc(sp.tmp_bytes))) return rc;
        sp.d_rec_off = sp.dsoff.as<uint64_t>();
        // the log between the two phases (one walk instead of two); without the memory for it the fill pass walks again
        sp.log_bytes = seed_log_bytes(n, ix->H().pos_bytes, kSeedLogSeedsDefault);
        if (sp.dlog.alloc(sp.log_bytes)) sp.log_bytes = 0;
        if (launch_marker_seeds_plan(ix->dev, ix->cfg, d_seqs, d_off, n, wsize, max_range, ftab_k, sp.dsoff.as<uint64_t>(), sp.dmoff.as<uint64_t>(), sp.dtmp.p, sp.tmp_bytes, st,
                                     sp.log_bytes ? sp.dlog.p : nullptr, sp.log_bytes))
            return RBG_ENODEV;
        if (h_seed_off) HIP_TRY(hipMemcpyAsync(h_seed_off, sp.dsoff.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        else HIP_TRY(hipMemcpyAsync(&sp.S, sp.dsoff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(&sp.total_mk, sp.dmoff.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!lmem && h_seed_off) sp.S = h_seed_off[n];
    return RBG_OK;
}

// Records and markers are allocated (DevBuf::alloc(0) is a block of 8 bytes: no pointer of an empty pass is null) and, when the pass has records, filled.
// Nothing is waited for: the caller's next step or copy-out follows on the stream.
int seed_pass_fill(rbg_index *ix, SeedPass &sp, hipStream_t st) {
    int rc;
    if ((rc = sp.dseeds.alloc(sp.S * sizeof(rbg_marker_seed_t))) || (rc = sp.dmk.alloc(sp.total_mk * 8))) return rc;
    if (sp.S == 0) return RBG_OK;
    uint64_t *seeds = sp.dseeds.as<uint64_t>(), *mk = sp.dmk.as<uint64_t>();
    const int e = sp.lmem ? launch_marker_lmems_fill(ix->dev, ix->cfg, sp.d_seqs, sp.d_off, sp.n, sp.S, sp.wsize, sp.max_range, sp.ftab_k, sp.dtmp.p, seeds, mk, st)
                          : launch_marker_seeds_fill(ix->dev, ix->cfg, sp.d_seqs, sp.d_off, sp.n, sp.wsize, sp.max_range, sp.ftab_k, sp.dsoff.as<uint64_t>(), sp.dmoff.as<uint64_t>(),
                                                     seeds, mk, st, sp.log_bytes ? sp.dlog.p : nullptr, sp.log_bytes);
    return e ? RBG_ENODEV : RBG_OK;
}

// A batch too big for one pass goes in passes of whole reads.  The end b of the pass that starts at read a: at least one read, then whole reads
// while they fit `chunk` (read bytes = lmem records per strand) and `max_reads`.
uint64_t pass_end(const uint64_t *off, uint64_t N, uint64_t a, uint64_t chunk, uint64_t max_reads = ~uint64_t(0)) {
    uint64_t b = a + 1;
    while (b < N && off[b + 1] - off[a] <= chunk && b - a < max_reads) ++b;
    return b;
}

// a pass's records index its own markers from 0: behind the mbase markers of the passes before, they move up
template <typename Rec>
void rebase_markers(Rec *recs, uint64_t count, uint64_t mbase) {
    for (uint64_t r = 0; mbase && r < count; ++r) { recs[r].mk_begin += mbase; recs[r].mk_end += mbase; }
}

// The argument checks and the launch of rbg_marker_seeds_plan_dev; rbg_marker_seeds_plan_log_dev checks its log and then comes here with it
int seeds_plan_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t max_range, uint64_t ftab_k, uint64_t *d_seed_off,
                   uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, void *stream, void *d_log = nullptr, size_t log_bytes = 0) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!d_seed_off || !d_mk_off || (N && (!d_seqs || !d_off))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    if (tmp_bytes < scan_tmp_bytes(N) || (N && !d_tmp)) return RBG_EARG;
    return launch_marker_seeds_plan(ix->dev, ix->cfg, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, d_tmp, tmp_bytes, stream, d_log, log_bytes) ? RBG_ENODEV : RBG_OK;
}

// the same for rbg_marker_seeds_fill_dev and rbg_marker_seeds_fill_log_dev
int seeds_fill_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t max_range, uint64_t ftab_k, const uint64_t *d_seed_off,
                   const uint64_t *d_mk_off, rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *stream, void *d_log = nullptr, size_t log_bytes = 0) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (N && (!d_seqs || !d_off || !d_seed_off || !d_mk_off || !d_seeds)) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    return launch_marker_seeds_fill(ix->dev, ix->cfg, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, reinterpret_cast<uint64_t *>(d_seeds), d_mk, stream, d_log,
                                    log_bytes) ? RBG_ENODEV : RBG_OK;
}

// what the two logged calls ask of their log: aligned, and room for two seeds per sequence
bool seed_log_ok(const rbg_index *ix, void *d_log, size_t log_bytes, uint64_t N) { return !N || make_seed_log(d_log, log_bytes, N, ix->H().pos_bytes).base; }
}  // namespace

extern "C" {
int rbg_markers_at(rbg_index *ix, const uint64_t *lo, const uint64_t *hi, uint64_t N, uint64_t *mk_off, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_ma) return RBG_ENOTLOADED;
    if (!mk_off || !mk || (N && (!lo || !hi))) return RBG_EARG;
    *mk = nullptr;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    DevBuf dlo, dhi, doff, dtmp;
    const size_t tmp_bytes = scan_tmp_bytes(N);
    int rc;
    if ((rc = dlo.alloc(N * 8)) || (rc = dhi.alloc(N * 8)) || (rc = doff.alloc((N + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes)))
        return rc;
    if (N) {
        HIP_TRY(hipMemcpyAsync(dlo.p, lo, N * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dhi.p, hi, N * 8, hipMemcpyHostToDevice, st));
    }
    if (launch_markers_plan(ix->dev, ix->cfg, dlo.as<uint64_t>(), dhi.as<uint64_t>(), N, doff.as<uint64_t>(), dtmp.p, tmp_bytes, st))
        return RBG_ENODEV;
    return ragged_finish(N, doff, mk_off, mk, st, [&](uint64_t *d_vals) {
        return launch_markers_fill(ix->dev, ix->cfg, dlo.as<uint64_t>(), dhi.as<uint64_t>(), N, doff.as<uint64_t>(), d_vals, st)
                   ? RBG_ENODEV : RBG_OK;
    });
    });
}

int rbg_find_range_w_markers(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize,
                             uint64_t max_range, uint64_t *lo, uint64_t *hi, uint64_t *mk_off, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_ma) return RBG_ENOTLOADED;  // reference: "warning: no marker array found!", default LFData
    if (!mk_off || !mk || wsize == 0 || (N && (!lo || !hi || !off))) return RBG_EARG;
    *mk = nullptr;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    ReadBatch rb;
    if ((rc = rb.stage(seqs, off, N, st))) return rc;
    DevBuf dlo, dhi, doff, dtmp;
    const size_t tmp_bytes = scan_tmp_bytes(N);
    if ((rc = dlo.alloc(N * 8)) || (rc = dhi.alloc(N * 8)) || (rc = doff.alloc((N + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes)))
        return rc;
    if (launch_find_range_markers_plan(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, wsize, max_range,
                                       dlo.as<uint64_t>(), dhi.as<uint64_t>(), doff.as<uint64_t>(), dtmp.p, tmp_bytes, st))
        return RBG_ENODEV;
    if (N) {
        HIP_TRY(hipMemcpyAsync(lo, dlo.p, N * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(hi, dhi.p, N * 8, hipMemcpyDeviceToHost, st));
    }
    return ragged_finish(N, doff, mk_off, mk, st, [&](uint64_t *d_vals) {
        return launch_find_range_markers_fill(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, wsize,
                                              max_range, doff.as<uint64_t>(), d_vals, st) ? RBG_ENODEV : RBG_OK;
    });
    });
}

// ---- marker seeds (next-row f4): get_markers_greedy_seeding, rowbowt.hpp:406-482 ---------------------

int rbg_marker_seeds_plan_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes,
                              void *stream) {
    return guarded([&]() -> int { return seeds_plan_dev(ix, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, d_tmp, tmp_bytes, stream); });
}

int rbg_marker_seeds_fill_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, const uint64_t *d_seed_off, const uint64_t *d_mk_off,
                              rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *stream) {
    return guarded([&]() -> int { return seeds_fill_dev(ix, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, d_seeds, d_mk, stream); });
}

// The same two phases with a LOG between them (rbg_dev.h SeedLog): the plan leaves every sequence's seed records and the
// places of its markers in d_log, the fill copies from there and walks only the sequences that exceeded their quota.
size_t rbg_marker_seeds_log_bytes(const rbg_index *ix, uint64_t N, uint32_t seeds_per_read) {
    if (!ix) return 0;
    if (seeds_per_read == 0) seeds_per_read = kSeedLogSeedsDefault;
    if (seeds_per_read < 2) seeds_per_read = 2;
    if (seeds_per_read > 255) seeds_per_read = 255;
    return seed_log_bytes(N, ix->H().pos_bytes, seeds_per_read);
}

int rbg_marker_seeds_plan_log_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                  uint64_t max_range, uint64_t ftab_k, uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes,
                                  void *d_log, size_t log_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!seed_log_ok(ix, d_log, log_bytes, N)) return RBG_EARG;
    return seeds_plan_dev(ix, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, d_tmp, tmp_bytes, stream, d_log, log_bytes);
    });
}

int rbg_marker_seeds_fill_log_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                  uint64_t max_range, uint64_t ftab_k, const uint64_t *d_seed_off, const uint64_t *d_mk_off,
                                  rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *d_log, size_t log_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    // (d_seeds: only here, not in rbg_marker_seeds_fill_dev: the logged fill copies 16-byte records, the walking fill writes words)
    if (reinterpret_cast<uintptr_t>(d_seeds) & 15 || !seed_log_ok(ix, d_log, log_bytes, N)) return RBG_EARG;
    return seeds_fill_dev(ix, d_seqs, d_off, N, wsize, max_range, ftab_k, d_seed_off, d_mk_off, d_seeds, d_mk, stream, d_log, log_bytes);
    });
}

static int marker_seeds_host(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize, uint64_t max_range,
                             uint64_t ftab_k, uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk) {
    int rc;
    *seeds = nullptr;
    *mk = nullptr;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    ReadBatch rb;
    SeedPass sp;
    if ((rc = rb.stage(seqs, off, N, st)) ||
        (rc = seed_pass_plan(ix, sp, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, N ? off[N] : 0, wsize, max_range, ftab_k, false, st, seed_off)))
        return rc;
    auto *h_seeds = static_cast<rbg_marker_seed_t *>(alloc_result(sp.S * sizeof(rbg_marker_seed_t)));
    auto *h_mk = static_cast<uint64_t *>(alloc_result(sp.total_mk * 8));
    rc = h_seeds && h_mk ? seed_pass_fill(ix, sp, st) : RBG_ENOMEM;
    if (!rc) rc = d2h_result(h_seeds, sp.dseeds.p, sp.S * sizeof(rbg_marker_seed_t), st);
    if (!rc) rc = d2h_result(h_mk, sp.dmk.p, sp.total_mk * 8, st);
    if (rc) { rbg_free_buffer(h_seeds); rbg_free_buffer(h_mk); return rc; }
    *seeds = h_seeds;
    *mk = h_mk;
    return RBG_OK;
}

struct SeedsReq : CombineReq {
    const uint8_t *seq = nullptr;
    uint64_t len = 0, wsize = 0, max_range = 0, ftab_k = 0;
    uint64_t nseeds = 0;
    rbg_marker_seed_t *seeds = nullptr;
    uint64_t *mk = nullptr;
};

// one read through the combiner (get_markers_greedy_seeding(query, wsize, max_range, fn) from a thread pool):
// requests with the same parameters share a launch; each gets its own slice, its marker offsets starting at 0
static int marker_seeds_one(rbg_index *ix, const uint8_t *seq, uint64_t len, uint64_t wsize, uint64_t max_range, uint64_t ftab_k,
                            uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk) {
    SeedsReq mine;
    mine.seq = seq; mine.len = len; mine.wsize = wsize; mine.max_range = max_range; mine.ftab_k = ftab_k;
    const int rc = combine_submit(ix, ix->comb_seeds, mine,
        [](const SeedsReq &a, const SeedsReq &b) { return a.wsize == b.wsize && a.max_range == b.max_range && a.ftab_k == b.ftab_k; },
        [&](std::vector<SeedsReq *> &batch) {
            const uint64_t K = batch.size();
            std::vector<uint64_t> off(K + 1, 0), soff(K + 1, 0);
            for (uint64_t i = 0; i < K; ++i) off[i + 1] = off[i] + batch[i]->len;
            std::vector<uint8_t> flat(off[K] + 1);
            for (uint64_t i = 0; i < K; ++i)
                if (batch[i]->len) std::memcpy(flat.data() + off[i], batch[i]->seq, batch[i]->len);
            rbg_marker_seed_t *all = nullptr;
            uint64_t *allmk = nullptr;
            int rc2 = marker_seeds_host(ix, flat.data(), off.data(), K, mine.wsize, mine.max_range, mine.ftab_k, soff.data(), &all, &allmk);
            if (!rc2 && K == 1) {   // nothing to split
                batch[0]->nseeds = soff[1];
                batch[0]->seeds = all;
                batch[0]->mk = allmk;
                all = nullptr;
                allmk = nullptr;
            } else if (!rc2) {
                for (uint64_t i = 0; i < K && !rc2; ++i) {
                    const uint64_t s0 = soff[i], s1 = soff[i + 1];
                    const uint64_t m0 = s1 > s0 ? all[s0].mk_begin : 0, m1 = s1 > s0 ? all[s1 - 1].mk_end : 0;
                    auto *hs = static_cast<rbg_marker_seed_t *>(std::malloc(std::max<size_t>(1, (s1 - s0) * sizeof(rbg_marker_seed_t))));
                    auto *hm = static_cast<uint64_t *>(std::malloc(std::max<size_t>(1, (m1 - m0) * 8)));
                    if (!hs || !hm) { std::free(hs); std::free(hm); rc2 = RBG_ENOMEM; break; }   // (plain malloc blocks)
                    for (uint64_t j = s0; j < s1; ++j) {
                        hs[j - s0] = all[j];
                        hs[j - s0].mk_begin -= m0;
                        hs[j - s0].mk_end -= m0;
                    }
                    if (m1 > m0) std::memcpy(hm, allmk + m0, (m1 - m0) * 8);
                    batch[i]->nseeds = s1 - s0;
                    batch[i]->seeds = hs;
                    batch[i]->mk = hm;
                }
            }
            rbg_free_buffer(all);
            rbg_free_buffer(allmk);
            if (rc2)
                for (SeedsReq *r : batch) { rbg_free_buffer(r->seeds); rbg_free_buffer(r->mk); r->seeds = nullptr; r->mk = nullptr; }
            for (SeedsReq *r : batch) r->rc = rc2;
        });
    if (rc) return rc;
    seed_off[0] = 0;
    seed_off[1] = mine.nseeds;
    *seeds = mine.seeds;
    *mk = mine.mk;
    return RBG_OK;
}

int rbg_get_markers_greedy_seeding(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize,
                                   uint64_t max_range, uint64_t ftab_k, uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!seed_off || !seeds || !mk || (N && !off)) return RBG_EARG;
    *seeds = nullptr;
    *mk = nullptr;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    if (N == 1 && combine_enabled()) return marker_seeds_one(ix, seqs, off[1], wsize, max_range, ftab_k, seed_off, seeds, mk);
    return marker_seeds_host(ix, seqs, off, N, wsize, max_range, ftab_k, seed_off, seeds, mk);
    });
}

// ---- lmem marker seeds: get_markers_lmems, rowbowt.hpp:341-404 -------------------------------------------------
// One record per (sequence, end position): record k of sequence i at off[i] - off[0] + k.  The plan walks every end position
// once to count its markers, scans those counts in d_tmp and writes the per-sequence scan; the fill walks again and writes.

size_t rbg_marker_lmems_tmp_bytes(uint64_t N, uint64_t total) {
    (void)N;
    return marker_lmems_tmp_bytes(total);
}

int rbg_marker_lmems_plan_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!d_mk_off || (N && (!d_seqs || !d_off || !d_tmp))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15 || reinterpret_cast<uintptr_t>(d_tmp) & 7) return RBG_EARG;
    if (N && tmp_bytes < marker_lmems_tmp_bytes(total)) return RBG_EARG;
    return launch_marker_lmems_plan(ix->dev, ix->cfg, d_seqs, d_off, N, total, wsize, max_range, ftab_k, d_mk_off, d_tmp, tmp_bytes, stream)
               ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_marker_lmems_fill_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t total, uint64_t wsize,
                              uint64_t max_range, uint64_t ftab_k, const void *d_tmp, rbg_marker_seed_t *d_seeds, uint64_t *d_mk, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (N && total && (!d_seqs || !d_off || !d_tmp || !d_seeds)) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15 || reinterpret_cast<uintptr_t>(d_tmp) & 7) return RBG_EARG;
    return launch_marker_lmems_fill(ix->dev, ix->cfg, d_seqs, d_off, N, total, wsize, max_range, ftab_k, d_tmp,
                                    reinterpret_cast<uint64_t *>(d_seeds), d_mk, stream) ? RBG_ENODEV : RBG_OK;
    });
}

// records per device pass of rbg_get_markers_lmems: 48 bytes each, 4 Mi records = 192 MiB of records plus 32 MiB of offsets
// (RBG_LMEM_CHUNK=<records> overrides; a sequence longer than a chunk gets a pass of its own)
static uint64_t lmem_chunk_records() {
    const char *e = std::getenv("RBG_LMEM_CHUNK");
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    return v ? v : (uint64_t(1) << 22);
}

int rbg_get_markers_lmems(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize, uint64_t max_range,
                          uint64_t ftab_k, uint64_t *seed_off, rbg_marker_seed_t **seeds, uint64_t **mk) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!seed_off || !seeds || !mk || (N && !off)) return RBG_EARG;
    *seeds = nullptr;
    *mk = nullptr;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    const uint64_t total = N ? off[N] : 0;
    for (uint64_t i = 0; i <= N; ++i) seed_off[i] = N ? off[i] : 0;   // exactly len(sequence) records each
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    auto *h_seeds = static_cast<rbg_marker_seed_t *>(alloc_result(total * sizeof(rbg_marker_seed_t)));
    if (!h_seeds) return RBG_ENOMEM;
    std::vector<uint64_t> h_mk;
    const uint64_t chunk = lmem_chunk_records();
    for (uint64_t a = 0; a < N && !rc;) {
        const uint64_t b = pass_end(off, N, a, chunk);   // (a sequence longer than the chunk gets a pass of its own)
        const uint64_t n = b - a, recs = off[b] - off[a];
        std::vector<uint64_t> roff(n + 1);
        for (uint64_t i = 0; i <= n; ++i) roff[i] = off[a + i] - off[a];
        ReadBatch rb;
        SeedPass sp;
        if ((rc = rb.stage(seqs + off[a], roff.data(), n, st)) ||
            (rc = seed_pass_plan(ix, sp, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), n, recs, wsize, max_range, ftab_k, true, st)) || (rc = seed_pass_fill(ix, sp, st)))
            break;
        rbg_marker_seed_t *dst = h_seeds + off[a];
        if ((rc = d2h_result(dst, sp.dseeds.p, recs * sizeof(rbg_marker_seed_t), st))) break;
        const uint64_t mbase = h_mk.size();
        h_mk.resize(mbase + sp.total_mk);
        if ((rc = d2h_result(h_mk.data() + mbase, sp.dmk.p, sp.total_mk * 8, st))) break;
        if (hipStreamSynchronize(st) != hipSuccess) { rc = RBG_ENODEV; break; }
        rebase_markers(dst, recs, mbase);
        a = b;
    }
    if (!rc) {
        *mk = static_cast<uint64_t *>(alloc_result(h_mk.size() * 8));
        if (!*mk) rc = RBG_ENOMEM;
        else if (!h_mk.empty()) std::memcpy(*mk, h_mk.data(), h_mk.size() * 8);
    }
    if (rc) { rbg_free_buffer(h_seeds); return rc; }
    *seeds = h_seeds;
    return RBG_OK;
    });
}

// ---- greedy seed lists (get_seeds_greedy :191-215, get_seeds_greedy_w_sample :222-256) and toehold checkpoints (:575-606) -------

size_t rbg_greedy_seeds_tmp_bytes(uint64_t N) { return scan_tmp_bytes(N); }

int rbg_greedy_seeds_plan_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length, uint32_t flags,
                              uint64_t *d_seed_off, void *d_tmp, size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if ((flags & ~RBG_SEEDS_W_SAMPLE) || !d_seed_off || (N && (!d_seqs || !d_off))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    if (tmp_bytes < scan_tmp_bytes(N) || (N && !d_tmp)) return RBG_EARG;
    const bool w_sample = (flags & RBG_SEEDS_W_SAMPLE) != 0;
    if (w_sample && !ix->H().has_tsa)   // rowbowt.hpp:225: every list is empty
        return hipMemsetAsync(d_seed_off, 0, (N + 1) * 8, static_cast<hipStream_t>(stream)) == hipSuccess ? RBG_OK : RBG_ENODEV;
    return launch_greedy_seeds_plan(ix->dev, ix->cfg, d_seqs, d_off, N, min_length, w_sample, d_seed_off, d_tmp, tmp_bytes, stream) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_greedy_seeds_fill_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length, uint32_t flags,
                              const uint64_t *d_seed_off, uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend,
                              uint64_t *d_ssamp, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    const bool w_sample = (flags & RBG_SEEDS_W_SAMPLE) != 0;
    if ((flags & ~RBG_SEEDS_W_SAMPLE) || !d_seed_off || (N && (!d_seqs || !d_off))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    if (w_sample && !ix->H().has_tsa) return RBG_OK;   // (the plan left every list empty)
    if (N && (!d_lo || !d_hi || !d_qstart || !d_qend || (w_sample && !d_ssamp))) return RBG_EARG;
    return launch_greedy_seeds_fill(ix->dev, ix->cfg, d_seqs, d_off, N, min_length, w_sample, d_seed_off, d_lo, d_hi, d_qstart, d_qend, d_ssamp, stream)
               ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_get_seeds_greedy(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length, uint32_t flags,
                         uint64_t *seed_off, uint64_t **seeds) {
    return guarded([&]() -> int {
    if (!seed_off || !seeds) return RBG_EARG;
    *seeds = nullptr;
    if (!queryable(ix)) return RBG_ENODEV;
    if ((flags & ~RBG_SEEDS_W_SAMPLE) || (N && !off)) return RBG_EARG;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    const bool w_sample = (flags & RBG_SEEDS_W_SAMPLE) != 0;
    if (w_sample && !ix->H().has_tsa) {   // rowbowt.hpp:225
        std::fill(seed_off, seed_off + N + 1, uint64_t(0));
        *seeds = static_cast<uint64_t *>(alloc_result(0));
        return *seeds ? RBG_OK : RBG_ENOMEM;
    }
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    ReadBatch rb;
    if ((rc = rb.stage(seqs, off, N, st))) return rc;
    DevBuf dsoff, dtmp, dout;
    const size_t tmp_bytes = scan_tmp_bytes(N);
    if ((rc = dsoff.alloc((N + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
    if (launch_greedy_seeds_plan(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, min_length, w_sample, dsoff.as<uint64_t>(), dtmp.p,
                                 tmp_bytes, st))
        return RBG_ENODEV;
    HIP_TRY(hipMemcpyAsync(seed_off, dsoff.p, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t total = seed_off[N];
    auto *h = static_cast<uint64_t *>(alloc_result(total * 40));
    if (!h) return RBG_ENOMEM;
    if (total) {
        if (!(rc = dout.alloc(total * 40))) {
            uint64_t *d = dout.as<uint64_t>();
            if (launch_greedy_seeds_fill(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, min_length, w_sample, dsoff.as<uint64_t>(), d,
                                         d + total, d + 2 * total, d + 3 * total, d + 4 * total, st))
                rc = RBG_ENODEV;
            if (!rc) rc = d2h_result(h, dout.p, total * 40, st);
        }
    }
    if (rc) { rbg_free_buffer(h); return rc; }
    *seeds = h;
    return RBG_OK;
    });
}

size_t rbg_toehold_chkpnts_tmp_bytes(uint64_t N) { return scan_tmp_bytes(N); }

int rbg_toehold_chkpnts_slots_dev(rbg_index *ix, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t *d_slot_off, void *d_tmp,
                                  size_t tmp_bytes, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (wsize == 0 || !d_slot_off || (N && !d_off)) return RBG_EARG;
    if (tmp_bytes < scan_tmp_bytes(N) || (N && !d_tmp)) return RBG_EARG;
    return launch_toehold_chkpnts_slots(ix->cfg, d_off, N, wsize, d_slot_off, d_tmp, tmp_bytes, stream) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_find_range_w_toehold_chkpnts_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize,
                                         const uint64_t *d_slot_off, uint64_t *d_cnt, uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart,
                                         uint64_t *d_qend, uint64_t *d_ssamp, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (wsize == 0) return RBG_EARG;
    if (N && (!d_seqs || !d_off || !d_slot_off || !d_cnt || !d_lo || !d_hi || !d_qstart || !d_qend || !d_ssamp)) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    return launch_toehold_chkpnts(ix->dev, ix->cfg, d_seqs, d_off, N, wsize, d_slot_off, d_cnt, d_lo, d_hi, d_qstart, d_qend, d_ssamp, stream)
               ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_find_range_w_toehold_chkpnts(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t wsize, uint64_t *seed_off,
                                     uint64_t **seeds) {
    return guarded([&]() -> int {
    if (!seed_off || !seeds) return RBG_EARG;
    *seeds = nullptr;
    if (!queryable(ix)) return RBG_ENODEV;
    if (wsize == 0 || (N && !off)) return RBG_EARG;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    std::fill(seed_off, seed_off + N + 1, uint64_t(0));
    if (!ix->H().has_tsa || N == 0) {   // rowbowt.hpp:579
        *seeds = static_cast<uint64_t *>(alloc_result(0));
        return *seeds ? RBG_OK : RBG_ENOMEM;
    }
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    ReadBatch rb;
    if ((rc = rb.stage(seqs, off, N, st))) return rc;
    DevBuf dsoff, dcnt, dtmp, dout;
    const size_t tmp_bytes = scan_tmp_bytes(N);
    if ((rc = dsoff.alloc((N + 1) * 8)) || (rc = dcnt.alloc(N * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
    if (launch_toehold_chkpnts_slots(ix->cfg, rb.off.as<uint64_t>(), N, wsize, dsoff.as<uint64_t>(), dtmp.p, tmp_bytes, st)) return RBG_ENODEV;
    std::vector<uint64_t> slot_off(N + 1), cnt(N);
    HIP_TRY(hipMemcpyAsync(slot_off.data(), dsoff.p, (N + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t slots = slot_off[N];
    std::vector<uint64_t> fixed(slots * 5);
    if (slots) {
        if ((rc = dout.alloc(slots * 40))) return rc;
        uint64_t *d = dout.as<uint64_t>();
        if (launch_toehold_chkpnts(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, wsize, dsoff.as<uint64_t>(), dcnt.as<uint64_t>(), d,
                                   d + slots, d + 2 * slots, d + 3 * slots, d + 4 * slots, st))
            return RBG_ENODEV;
        HIP_TRY(hipMemcpyAsync(cnt.data(), dcnt.p, N * 8, hipMemcpyDeviceToHost, st));
        if ((rc = d2h_result(fixed.data(), dout.p, slots * 40, st))) return rc;
    }
    // compact: the slots of the reads that occur, in read order
    for (uint64_t i = 0; i < N; ++i) seed_off[i + 1] = seed_off[i] + (slots ? cnt[i] : 0);
    const uint64_t total = seed_off[N];
    auto *h = static_cast<uint64_t *>(alloc_result(total * 40));
    if (!h) return RBG_ENOMEM;
    for (uint64_t i = 0; i < N; ++i) {
        const uint64_t c = seed_off[i + 1] - seed_off[i];
        for (int a = 0; a < 5; ++a)
            std::copy_n(fixed.data() + a * slots + slot_off[i], c, h + a * total + seed_off[i]);
    }
    *seeds = h;
    return RBG_OK;
    });
}

// ---- greedy seeding (next-row f4) -----------------------------------------------------------------

int rbg_greedy_longest_seed_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length,
                                uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend, uint64_t *d_ssamp,
                                void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (N && (!d_seqs || !d_off || !d_lo || !d_hi || !d_qstart || !d_qend || !d_ssamp)) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    return launch_greedy_seed(ix->dev, ix->cfg, d_seqs, d_off, N, min_length, d_lo, d_hi, d_qstart, d_qend, d_ssamp, stream)
               ? RBG_ENODEV : RBG_OK;
    });
}

// The instrumented instantiations of the seeding kernels (run-indexed layout; include/rbg.h RBG_SEED_STATS): the same walks and outputs, plus what
// they touched.  bench.py prices the kernels' rooflines from these sums.
int rbg_greedy_longest_seed_stats_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t min_length,
                                      uint64_t *d_lo, uint64_t *d_hi, uint64_t *d_qstart, uint64_t *d_qend, uint64_t *d_ssamp, uint64_t *d_stats,
                                      void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (!d_stats || (N && (!d_seqs || !d_off || !d_lo || !d_hi || !d_qstart || !d_qend || !d_ssamp))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    if (ix->dev.layout != RBG_LAYOUT_RUNS) return RBG_EARG;
    return launch_greedy_seed(ix->dev, ix->cfg, d_seqs, d_off, N, min_length, d_lo, d_hi, d_qstart, d_qend, d_ssamp, stream,
                              reinterpret_cast<unsigned long long *>(d_stats)) ? RBG_ENODEV : RBG_OK;
    });
}

// plan (count walk + scans) and fill (second walk) of the marker seeds in one call, both instrumented, sums added to d_stats
int rbg_marker_seeds_stats_dev(rbg_index *ix, const uint8_t *d_seqs, const uint64_t *d_off, uint64_t N, uint64_t wsize, uint64_t max_range,
                               uint64_t *d_seed_off, uint64_t *d_mk_off, void *d_tmp, size_t tmp_bytes, rbg_marker_seed_t *d_seeds, uint64_t *d_mk,
                               uint64_t *d_stats, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!d_stats || !d_seed_off || !d_mk_off || (N && (!d_seqs || !d_off || !d_seeds))) return RBG_EARG;
    if (reinterpret_cast<uintptr_t>(d_seqs) & 15) return RBG_EARG;
    if (tmp_bytes < scan_tmp_bytes(N) || (N && !d_tmp)) return RBG_EARG;
    if (ix->dev.layout != RBG_LAYOUT_RUNS) return RBG_EARG;
    unsigned long long *st = reinterpret_cast<unsigned long long *>(d_stats);
    if (launch_marker_seeds_plan(ix->dev, ix->cfg, d_seqs, d_off, N, wsize, max_range, 0, d_seed_off, d_mk_off, d_tmp, tmp_bytes, stream, nullptr, 0, st)) return RBG_ENODEV;
    return launch_marker_seeds_fill(ix->dev, ix->cfg, d_seqs, d_off, N, wsize, max_range, 0, d_seed_off, d_mk_off, reinterpret_cast<uint64_t *>(d_seeds), d_mk,
                                    stream, nullptr, 0, st) ? RBG_ENODEV : RBG_OK;
    });
}

int rbg_locate_fill_offset_dev(rbg_index *ix, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N,
                               uint64_t max_hits, const uint64_t *d_loc_off, uint64_t *d_locs, const uint64_t *d_sub,
                               const void *d_order, void *stream) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (N && (!d_lo || !d_hi || !d_k || !d_loc_off || !d_locs)) return RBG_EARG;
    return launch_locate_fill(ix->dev, ix->cfg, d_lo, d_hi, d_k, N, max_hits, d_loc_off, d_locs, d_sub, d_order, stream) ? RBG_ENODEV : RBG_OK;
    });
}

// behind K3's fill, while the locations are still on the device (d_locs, d_loc_off, the reads' d_off): what rbg_find_loc_markers_greedy_seeding hangs on
typedef std::function<int(const uint64_t *, const uint64_t *, const uint64_t *, hipStream_t)> AfterLocate;
static int greedy_host(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                       uint64_t *lo, uint64_t *hi, uint64_t *qs, uint64_t *qe, uint64_t *ss, bool locate, uint64_t max_hits,
                       uint64_t *loc_off, uint64_t **locs, const AfterLocate *after = nullptr) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (N && !off) return RBG_EARG;
    int rc = check_offsets(off, N);
    if (rc) return rc;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    ReadBatch rb;
    if ((rc = rb.stage(seqs, off, N, st))) return rc;
    DevBuf d[5], doff, dtmp;
    for (auto &b : d)
        if ((rc = b.alloc(N * 8))) return rc;
    if (launch_greedy_seed(ix->dev, ix->cfg, rb.seqs.as<uint8_t>(), rb.off.as<uint64_t>(), N, min_length, d[0].as<uint64_t>(),
                           d[1].as<uint64_t>(), d[2].as<uint64_t>(), d[3].as<uint64_t>(), d[4].as<uint64_t>(), st))
        return RBG_ENODEV;
    uint64_t *outs[5] = {lo, hi, qs, qe, ss};
    for (int a = 0; a < 5; ++a)
        if (outs[a] && N) HIP_TRY(hipMemcpyAsync(outs[a], d[a].p, N * 8, hipMemcpyDeviceToHost, st));
    if (!locate) {
        HIP_TRY(hipStreamSynchronize(st));
        return RBG_OK;
    }
    const size_t tmp_bytes = scan_tmp_bytes(N);
    if ((rc = doff.alloc((N + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes))) return rc;
    if (launch_locate_plan(ix->dev, ix->cfg, d[0].as<uint64_t>(), d[1].as<uint64_t>(), N, max_hits, doff.as<uint64_t>(), dtmp.p, tmp_bytes, st))
        return RBG_ENODEV;
    DevBuf dord;
    const void *order = nullptr;
    if ((rc = make_order(ix, d[4].as<uint64_t>(), N, dord, st, &order))) return rc;
    return ragged_finish(N, doff, loc_off, locs, st, [&](uint64_t *d_vals) {
        if (launch_locate_fill(ix->dev, ix->cfg, d[0].as<uint64_t>(), d[1].as<uint64_t>(), d[4].as<uint64_t>(), N, max_hits,
                               doff.as<uint64_t>(), d_vals, d[2].as<uint64_t>(), order, st)) return static_cast<int>(RBG_ENODEV);
        return after ? (*after)(d_vals, doff.as<uint64_t>(), rb.off.as<uint64_t>(), st) : static_cast<int>(RBG_OK);
    });
}

int rbg_greedy_longest_seed(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                            uint64_t *lo, uint64_t *hi, uint64_t *qstart, uint64_t *qend, uint64_t *ssamp) {
    return guarded([&]() -> int {
    if (N && (!lo || !hi || !qstart || !qend || !ssamp)) return RBG_EARG;
    return greedy_host(ix, seqs, off, N, min_length, lo, hi, qstart, qend, ssamp, false, 0, nullptr, nullptr);
    });
}

int rbg_find_locs_greedy_seeding(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t min_length,
                                 uint64_t max_hits, uint64_t *loc_off, uint64_t **locs) {
    return guarded([&]() -> int {
    if (!loc_off || !locs) return RBG_EARG;
    *locs = nullptr;
    return greedy_host(ix, seqs, off, N, min_length, nullptr, nullptr, nullptr, nullptr, nullptr, true, max_hits, loc_off, locs);
    });
}

}  // extern "C"
