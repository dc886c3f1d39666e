// capi/upload_runs.ipp -- the run-indexed layout: its tables on the device (run lists, fillers, folded F, directories / bucket records, phi), and the
// composition of the k-mer depths on the device.  Part of rbg_capi.hip.
namespace {
// ---- the run-indexed layout (rbg_dev.h DevRunTab2; kernels: rbg_runs2_device.hpp) ---------------------------------------
// Inputs: the depth-1 tables of the host index and the k-mer levels composed on the device.
// Everything but the conversion of the depth-1 lists happens in kernels (k_build.hip): fillers (8-byte positions, only
// where a table has a gap of 2^30 rows or more), the low-word pairs, the directories, the phi list, its directory and
// super counts.  Nothing is left out for its size: entry indices are 64-bit, a table may hold up to 2^32 - 16 entries
// (more is an error with a message, not a silent drop), and the phi directory has no size cap.
struct TmpDev {   // device scratch of the load, freed at scope exit
    void *p = nullptr;
    ~TmpDev() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV; }
        return RBG_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    template <typename T> T *as() { return static_cast<T *>(p); }
};
inline size_t scan_tmp_bytes_for(uint64_t N) { return scan_tmp_bytes(N); }

// fillers for a list of m {key, value} u64 pairs at *ent (device; tables closed by sentinels with key n).  When some are
// needed: *ent / *samp are replaced by the expanded arrays (`own` says whether the old ones are tracked allocations of the
// index or plain hipMalloc blocks), *m by the new count, and `at` (indices into the old list) by their new places.
int add_fillers(rbg_index *ix, bool phi, void **ent, void **samp, bool tracked, uint64_t *m, uint64_t n, std::vector<uint64_t> &at, uint64_t *fillers) {
    *fillers = 0;
    const uint32_t fs = ix->dev.run_fill_shift;
    TmpDev tot;
    int rc = tot.alloc(8);
    if (rc) return rc;
    HIP_TRY(hipMemset(tot.p, 0, 8));
    HIP_TRY(static_cast<hipError_t>(launch_fill_count(*ent, *m, n, fs, nullptr, tot.as<unsigned long long>(), nullptr)));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpy(&total, tot.p, 8, hipMemcpyDeviceToHost));
    if (!total) return RBG_OK;
    if (total > (uint64_t(1) << 40) || *m > (uint64_t(1) << 40)) return RBG_ENOMEM;   // (sizes below stay far from 2^64; no index that fits a device comes near)
    TmpDev arr, tmp, idx, out;
    const size_t tb = scan_tmp_bytes_for(*m + 1);
    if ((rc = arr.alloc((*m + 1) * 8)) || (rc = tmp.alloc(tb))) return rc;
    HIP_TRY(hipMemset(tot.p, 0, 8));
    HIP_TRY(static_cast<hipError_t>(launch_fill_count(*ent, *m, n, fs, arr.as<uint64_t>(), tot.as<unsigned long long>(), nullptr)));
    HIP_TRY(static_cast<hipError_t>(launch_scan_u64(arr.as<uint64_t>(), *m + 1, tmp.p, tb, nullptr)));
    const uint64_t m2 = *m + total;
    // the expanded arrays: given back on EVERY error path below (a tracked block through the index's list, a plain one by hipFree),
    // handed to the caller only once everything has succeeded
    struct NewBlock {
        rbg_index *ix; bool tracked; void *p = nullptr;
        NewBlock(rbg_index *i, bool t) : ix(i), tracked(t) {}
        ~NewBlock() { if (!p) return; if (tracked) free_tracked(ix, p); else (void)hipFree(p); }
        int alloc(size_t bytes) {
            if (tracked) {
                // (its own allocation, never a piece of the arena: free_tracked must be able to give it back)
                hipError_t e = hipMalloc(&p, arena_round(bytes));
                if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV; }
                ix->allocs.push_back({p, arena_round(bytes)});
                ix->hbm_bytes += arena_round(bytes);
                return RBG_OK;
            }
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV; }
            return RBG_OK;
        }
        void *release() { void *q = p; p = nullptr; return q; }
    } ent2(ix, tracked), samp2(ix, tracked);
    if ((rc = ent2.alloc((m2 + 2) * 16))) return rc;
    if (*samp && (rc = samp2.alloc(m2 * 8 + 16))) return rc;
    HIP_TRY(static_cast<hipError_t>(launch_fill_expand(phi, *ent, static_cast<const uint64_t *>(*samp), *m, n, fs, arr.as<uint64_t>(), ent2.p, static_cast<uint64_t *>(samp2.p), nullptr)));
    if (!at.empty()) {
        if ((rc = idx.alloc(at.size() * 8)) || (rc = out.alloc(at.size() * 8))) return rc;
        HIP_TRY(hipMemcpy(idx.p, at.data(), at.size() * 8, hipMemcpyHostToDevice));
        HIP_TRY(static_cast<hipError_t>(launch_gather_u64(arr.as<uint64_t>(), idx.as<uint64_t>(), at.size(), out.as<uint64_t>(), nullptr)));
        HIP_TRY(hipMemcpy(at.data(), out.p, at.size() * 8, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (tracked) { free_tracked(ix, *ent); if (*samp) free_tracked(ix, *samp); }
    else { (void)hipFree(*ent); if (*samp) (void)hipFree(*samp); }
    *ent = ent2.release();
    *samp = samp2.release();
    *m = m2;
    *fillers = total;
    return RBG_OK;
}

// ---- upload_tables_runs2: what a load of the run-indexed layout puts on the device, step by step ------------------------------------------------------
// The geometry rules (bucket shifts, the uniform depth, the phi slots and directory, the stage tables) are rbg_load_plan.hpp's; here are the device
// allocations, copies and kernel launches, in an order hbm_bytes, the arena's contents and the replicas' allocation list depend on.

// The switches of one load, read ONCE PER LOAD (tests change them between loads) and nowhere below.
struct RunSwitches {
    double dir_target;     // RBG_RANK_DIR_RUNS: runs per directory bucket at most this on average (default 4)
    double rec_asked;      // RBG_RUN_REC_PER: entries per record bucket on average (0: run_record_plan's 2.5 / 4 / 6)
    int uniform;           // RBG_RUN_UNIFORM: 0 / 1 = never / whenever the depth is deep enough (tests, A/B); -1: unset
    double phi_per;        // RBG_PHI_DIR_PER: sampled positions per phi directory bucket at least this on average (default 1)
    uint32_t fill_shift, super_shift;   // RBG_RUN_FILL_SHIFT / RBG_PHI_SUPER_SHIFT: test-only, so that small indexes meet fillers and several super blocks
    bool verbose;          // RBG_VERBOSE
};
inline RunSwitches read_run_switches() {
    auto positive = [](const char *name, double dflt) { const char *e = std::getenv(name); return e && std::atof(e) > 0 ? std::atof(e) : dflt; };
    RunSwitches s;
    s.dir_target = positive("RBG_RANK_DIR_RUNS", 4.0);
    s.fill_shift = static_cast<uint32_t>(env_opt("RBG_RUN_FILL_SHIFT", kRunFillShift, 4, kRunFillShift));
    s.super_shift = static_cast<uint32_t>(env_opt("RBG_PHI_SUPER_SHIFT", kPhiSuperShift, 1, 24));
    s.rec_asked = positive("RBG_RUN_REC_PER", 0.0);
    const char *e_uni = std::getenv("RBG_RUN_UNIFORM");
    s.uniform = e_uni ? std::atoi(e_uni) : -1;
    s.phi_per = positive("RBG_PHI_DIR_PER", 1.0);
    s.verbose = std::getenv("RBG_VERBOSE") != nullptr;
    return s;
}

// what the steps of one load share
struct RunLoad {
    rbg_index *ix;
    HostIndex &h;
    RunSwitches sw;
    LoadConsts consts;
    bool wide;                       // 8-byte positions
    uint32_t D = 1, mask = 1;        // the depths composed; bit d - 1: depth d keeps its run lists
    uint32_t max_shift = 31;         // of a bucket (a per-lane shift of the low word: rbg_device.hpp pos_bucket)
    std::vector<double> rec_per;     // [d]: entries per bucket on average of depth d + 1's records, 0 = directories (rbg_load_plan.hpp run_record_plan)
    std::vector<DevRunTab2> tabs;    // the table records of every depth so far, each depth closed by one more
    std::vector<uint64_t> hot;       // rbg_dev.h: dir_off | dir_shift << 56 per table
    RunLoad(rbg_index *ix_, bool wide_) : ix(ix_), h(ix_->H()), sw(read_run_switches()), consts(load_consts()), wide(wide_) {}
};
// the buckets of a depth's tables: table t's shift, and its first bucket (directory entry or record) among the depth's; off[tables]: all of them
struct TableBuckets {
    std::vector<uint32_t> shift;
    std::vector<uint64_t> off;
};
// what the steps of one kept depth share
struct RunDepth {
    uint32_t d;                                    // the depth's index: k-mer depth d + 1
    const std::vector<SymTable> &T;
    std::vector<uint64_t> first, nr;               // table t's first entry among the depth's, and its entries without the sentinel; first[tables]: all of them
    TableBuckets b;
    void *abs_ent = nullptr, *abs_samp = nullptr;  // the depth's {start, cum} pairs of P, tables back to back, and its samples (P each)
    uint64_t E2 = 0, fillers = 0;                  // entries with the fillers; the fillers
    RunDepth(uint32_t d_, const std::vector<SymTable> &T_) : d(d_), T(T_), first(T_.size() + 1, 0), nr(T_.size()) {
        for (size_t t = 0; t < T.size(); ++t) { first[t + 1] = first[t] + T[t].nruns + 1; nr[t] = T[t].nruns; }
        E2 = first[T.size()];
    }
    size_t nt() const { return T.size(); }
    uint64_t buckets() const { return b.off[nt()]; }
    // per table the widest bucket that still holds at most about `per` entries on average (rbg_load_plan.hpp bucket_shift)
    void own_buckets(double per, uint64_t n, uint32_t max_shift) {
        b.shift.assign(nt(), 0);
        b.off.assign(nt() + 1, 0);
        for (size_t t = 0; t < nt(); ++t) {
            b.shift[t] = bucket_shift(static_cast<double>(nr[t]), per, n, max_shift);
            b.off[t + 1] = b.off[t] + bucket_count(n, b.shift[t]);
        }
    }
};

// the depth-1 lists compose_on_device left on the device are the slot layout's
void release_slot_lists(rbg_index *ix) {
    for (SymTable &t : ix->H().sym) {
        free_tracked(ix, const_cast<void *>(t.dev_ent));
        free_tracked(ix, const_cast<void *>(t.dev_samp));
        t.dev_ent = t.dev_samp = nullptr;
    }
}

// the depths composed, those that keep their run lists, and which of them get bucket records
void settle_depths(RunLoad &L, const std::vector<SymTable> *depth[kMaxRunDepth]) {
    rbg_index *ix = L.ix;
    depth[0] = &L.h.sym;
    for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxRunDepth); ++d) depth[d - 1] = &L.h.kmer(d);
    while (L.D < static_cast<uint32_t>(kMaxRunDepth) && !depth[L.D]->empty()) ++L.D;
    ix->runs_report.depths_composed = L.D;
    L.mask = (ix->run_depth_mask ? ix->run_depth_mask : ~0u) & ((1u << L.D) - 1u);
    L.mask |= 1u | (1u << (L.D - 1));   // (the deepest is always kept: the kernels step by it)
    ix->dev.run_fill_shift = L.sw.fill_shift;
    L.max_shift = L.wide ? ix->dev.run_fill_shift : 31u;
    // BUCKET RECORDS (RBG_OPT_RUN_REC; rbg_dev.h RunRec2): one aligned 64-byte record per bucket of about three entries instead of
    // the directory -- a rank is one sector.  Automatic: when all kept depths with their records (about 64 / 3 bytes per entry) and
    // the rest of the replica stay within half the budget.  RBG_RUN_REC_PER: entries per bucket on average (default 2.5 inside the
    // bucket; the one before them is held too).  Per depth, deepest first: rbg_load_plan.hpp run_record_plan.
    L.rec_per = run_record_plan(shape_of(L.h), L.consts, L.mask, L.D, ix->hbm_budget, g_opt_run_rec.load(), g_opt_run_rec_depths.load(), L.sw.rec_asked, L.max_shift,
                                g_opt_run_phi.load());
}

// a depth without run lists: nothing steps by it
void leave_depth_out(RunLoad &L, uint32_t d) {
    release_kmer_level(L.ix, d + 1);
    for (SymTable &st : kmer_level_tables(L.h, d + 1)) st.dev_ent = st.dev_samp = nullptr;
}

// the depth's lists converted from the host tables and copied to the device
template <typename P>
int convert_host_tables(RunLoad &L, RunDepth &R) {
    const HostIndex &h = L.h;
    const std::vector<SymTable> &T = R.T;
    const uint64_t entries = R.E2;
    HostBuf<RunEnt<P>> ent(entries + 2);
    HostBuf<P> samp(h.has_tsa ? entries + 2 : 0);
    const size_t Wk = std::max<size_t>(1, std::min<size_t>({16, std::thread::hardware_concurrency(), T.size()}));
    std::vector<std::thread> workers;
    for (size_t w = 0; w < Wk; ++w)
        workers.emplace_back([&, w] {
            for (size_t t = w; t < T.size(); t += Wk) {
                const SymTable &tb = T[t];
                if (tb.start.size() != tb.nruns + 1) continue;   // (checked below)
                for (uint64_t k = 0; k <= tb.nruns; ++k) ent[R.first[t] + k] = RunEnt<P>{static_cast<P>(tb.start[k]), static_cast<P>(tb.cum[k])};
                if (h.has_tsa) {
                    for (uint64_t k = 0; k < tb.nruns; ++k) samp[R.first[t] + k] = static_cast<P>(tb.samp[k]);
                    samp[R.first[t] + tb.nruns] = 0;
                }
            }
        });
    for (auto &w : workers) w.join();
    for (const SymTable &tb : T)
        if (tb.start.size() != tb.nruns + 1) return RBG_EARG;   // a table without host arrays and without a device level
    for (uint64_t x = 0; x < 2; ++x) { ent[entries + x] = ent[entries - 1]; if (h.has_tsa) samp[entries + x] = 0; }
    const void *up = nullptr;
    int rc;
    if ((rc = dev_upload(L.ix, ent.data(), (entries + 2) * sizeof(RunEnt<P>), &up))) return rc;
    R.abs_ent = const_cast<void *>(up);
    if (h.has_tsa) {
        if ((rc = dev_upload(L.ix, samp.data(), (entries + 2) * sizeof(P), &up))) return rc;
        R.abs_samp = const_cast<void *>(up);
    }
    return RBG_OK;
}

// the depth's {start, cum} pairs and samples on the device: the level composed there is adopted, else the host tables are converted
template <typename P>
int depth_lists_on_device(RunLoad &L, RunDepth &R) {
    rbg_index *ix = L.ix;
    const uint32_t d = R.d;
    ComposedLevel *lv = (d >= 1 && d - 1 < ix->kmer_levels.size() && ix->kmer_levels[d - 1].ent) ? &ix->kmer_levels[d - 1] : nullptr;
    if (!lv) return convert_host_tables<P>(L, R);
    if (lv->entries != R.E2 || lv->first.size() != R.nt()) return RBG_EARG;
    for (size_t t = 0; t < R.nt(); ++t)
        if (lv->first[t] != R.first[t]) return RBG_EARG;
    R.abs_ent = lv->ent;
    R.abs_samp = L.h.has_tsa ? lv->samp : nullptr;
    lv->ent = lv->samp = nullptr;   // (adopted: the index's allocation list keeps them)
    return RBG_OK;
}

// fillers (8-byte positions only: add_fillers), then the limit a table's entries must stay under
template <typename P>
int depth_fillers(RunLoad &L, RunDepth &R) {
    if constexpr (sizeof(P) == 8) {
        std::vector<uint64_t> at;
        for (size_t t = 0; t < R.nt(); ++t) { at.push_back(R.first[t]); at.push_back(R.first[t] + R.nr[t]); }
        if (const int rc = add_fillers(L.ix, false, &R.abs_ent, &R.abs_samp, true, &R.E2, L.h.n, at, &R.fillers)) return rc;
        if (R.fillers) {
            for (size_t t = 0; t < R.nt(); ++t) { R.first[t] = at[2 * t]; R.nr[t] = at[2 * t + 1] - at[2 * t]; }
            R.first[R.nt()] = R.E2;
        }
    }
    for (size_t t = 0; t < R.nt(); ++t)
        if (R.nr[t] >= 0xFFFFFFF0ull) {
            std::fprintf(stderr, "rbg: a table of k-mer depth %u has %llu entries: the run-indexed layout holds fewer than 2^32 - 16 per table\n", R.d + 1,
                         static_cast<unsigned long long>(R.nr[t]));
            return RBG_EARG;
        }
    L.ix->runs_report.entries[R.d] = R.E2;
    L.ix->runs_report.fillers[R.d] = R.fillers;
    return RBG_OK;
}

// every cum becomes a ROW of the F column: + the table's F (rbg_dev.h kRunHotShiftBit; k_build.hip k_fold_F)
template <typename P>
int fold_F(RunLoad &L, RunDepth &R) {
    TmpDev tf;
    const size_t nt = R.nt();
    if (const int rc = tf.alloc((2 * nt + 1) * 8)) return rc;
    std::vector<uint64_t> Fv(nt);
    for (size_t t = 0; t < nt; ++t) Fv[t] = R.T[t].F;
    uint64_t *t_first = tf.as<uint64_t>(), *t_F = t_first + nt + 1;
    HIP_TRY(hipMemcpy(t_first, R.first.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t_F, Fv.data(), nt * 8, hipMemcpyHostToDevice));
    // (4-byte positions: the two spare entries are final too)
    HIP_TRY(static_cast<hipError_t>(launch_fold_F(sizeof(P), R.abs_ent, t_first, t_F, static_cast<uint32_t>(nt), R.E2 + (sizeof(P) == 8 ? 0 : 2), nullptr)));
    HIP_TRY(hipDeviceSynchronize());
    return RBG_OK;
}

// the per-table geometry of a depth (first, nr, b.off, b.shift) in device scratch: what the directory and the record kernels read
struct DevTableGeometry {
    TmpDev tmp;
    uint64_t *first = nullptr, *nr = nullptr, *off = nullptr;
    uint32_t *shift = nullptr;
    int upload(const RunDepth &R) {
        const size_t nt = R.nt();
        if (const int rc = tmp.alloc((3 * nt + 1) * 8 + nt * 4)) return rc;
        first = tmp.as<uint64_t>(), nr = first + nt, off = nr + nt;
        shift = reinterpret_cast<uint32_t *>(off + nt + 1);
        HIP_TRY(hipMemcpy(first, R.first.data(), nt * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(nr, R.nr.data(), nt * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(off, R.b.off.data(), (nt + 1) * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(shift, R.b.shift.data(), nt * 4, hipMemcpyHostToDevice));
        return RBG_OK;
    }
};

// directories: per table the widest bucket that still holds at most about dir_target entries on average
template <typename P>
int build_depth_directory(RunLoad &L, RunDepth &R) {
    constexpr bool W = sizeof(P) == 8;
    R.own_buckets(L.sw.dir_target, L.h.n, L.max_shift);
    void *dirp = nullptr;
    const size_t dir_ent = W ? sizeof(RunDir64) : 4;
    const uint32_t nt = static_cast<uint32_t>(R.nt());
    int rc;
    if ((rc = dev_reserve(L.ix, R.buckets() * dir_ent + 16, &dirp))) return rc;
    DevTableGeometry g;
    if ((rc = g.upload(R))) return rc;
    if constexpr (W) HIP_TRY(static_cast<hipError_t>(launch_run_dirs2(R.abs_ent, g.first, g.nr, g.off, g.shift, nt, R.buckets(), dirp, nullptr)));
    else HIP_TRY(static_cast<hipError_t>(launch_run_dirs(4, R.abs_ent, g.first, g.nr, g.off, g.shift, nt, R.buckets(), static_cast<uint32_t *>(dirp), nullptr)));
    HIP_TRY(hipDeviceSynchronize());
    L.ix->runs_report.dir_bytes[R.d] = R.buckets() * dir_ent;
    L.ix->dev.run_dir2[R.d] = dirp;
    return RBG_OK;
}

// the depth's bucket records under the buckets R.b as they stand: *recp, and how many overflow their record
template <typename P>
int build_records(RunLoad &L, RunDepth &R, void **recp, unsigned long long *novf) {
    int rc;
    if ((rc = dev_reserve(L.ix, R.buckets() * sizeof(RunRec2) + 64, recp))) return rc;
    DevTableGeometry g;
    TmpDev ovf;
    if ((rc = g.upload(R)) || (rc = ovf.alloc(8))) return rc;
    HIP_TRY(hipMemset(ovf.p, 0, 8));
    HIP_TRY(static_cast<hipError_t>(launch_run_recs2(sizeof(P), R.abs_ent, g.first, g.nr, g.off, g.shift, static_cast<uint32_t>(R.nt()), R.buckets(), *recp,
                                                     ovf.as<unsigned long long>(), nullptr)));
    HIP_TRY(hipMemcpy(novf, ovf.p, 8, hipMemcpyDeviceToHost));
    return RBG_OK;
}

// A uniform depth whose records overflow often (rbg_load_plan.hpp uniform_needs_comparison) against the tables' own buckets: the records are built under
// those, counted, and -- when uniform stays -- built a third time.  One record array at a time: two would raise the load's peak.
template <typename P>
int compare_uniform_with_own(RunLoad &L, RunDepth &R, const TableBuckets &own, void **recp, unsigned long long *novf, bool *uniform) {
    const TableBuckets uni = R.b;
    const unsigned long long novf_uni = *novf;
    int rc;
    free_tracked(L.ix, *recp);
    *recp = nullptr;
    R.b = own;
    if ((rc = build_records<P>(L, R, recp, novf))) return rc;
    const unsigned long long novf_own = *novf;
    if (uniform_stays(novf_uni, novf_own, uni.off[R.nt()])) {
        free_tracked(L.ix, *recp);
        *recp = nullptr;
        R.b = uni;
        return build_records<P>(L, R, recp, novf);
    }
    *uniform = false;
    if (L.sw.verbose)
        std::fprintf(stderr, "rbg:   depth %u: uniform directories would leave %llu records overflowing, the tables' own shifts %llu: the tables keep their own shifts\n",
                     R.d + 1, novf_uni, novf_own);
    return RBG_OK;
}

// bucket records instead of the directory: per table the widest bucket with at most rec_per[d] entries starting inside on average -- or, for the deepest
// depth beyond the LDS-staged ones, one shift and one record count for all its tables (rbg_load_plan.hpp uniform_candidate and the verdict after counting)
template <typename P>
int build_depth_records(RunLoad &L, RunDepth &R) {
    rbg_index *ix = L.ix;
    const uint32_t d = R.d;
    const size_t nt = R.nt();
    R.own_buckets(L.rec_per[d], L.h.n, L.max_shift);
    const TableBuckets own = R.b;
    double total_runs = 0;
    for (size_t t = 0; t < nt; ++t) total_runs += static_cast<double>(R.nr[t]);
    const UniformCandidate cand = uniform_candidate(deepest_with_records(L.rec_per, L.mask, d, L.D), d, nt, L.tabs.size(), total_runs, own.off[nt], L.rec_per[d], L.h.n,
                                                    L.max_shift, L.sw.uniform, L.consts);
    bool uniform = cand.eligible;
    if (uniform)
        for (size_t t = 0; t < nt; ++t) { R.b.shift[t] = cand.shift; R.b.off[t + 1] = R.b.off[t] + cand.stride; }
    void *recp = nullptr;
    unsigned long long novf = 0;
    int rc;
    if ((rc = build_records<P>(L, R, &recp, &novf))) return rc;
    if (uniform && uniform_needs_comparison(novf, R.buckets(), L.sw.uniform) && (rc = compare_uniform_with_own<P>(L, R, own, &recp, &novf, &uniform))) return rc;
    if (uniform) {
        const uint64_t stride = R.b.off[1] - R.b.off[0];
        if (!uniform_stride_fits(stride, L.consts)) return RBG_EARG;   // (load_run_tab's packed constants: a 27-bit stride, a 5-bit shift, a 24-bit first record)
        ix->dev.run_uni_depth = d; ix->dev.run_uni_stride = static_cast<uint32_t>(stride); ix->dev.run_uni_shift = R.b.shift[0];
        if (L.sw.verbose)
            std::fprintf(stderr, "rbg:   depth %u: uniform directories (shift %u, %llu records per table, %llu of %llu overflowing): hot words computed\n", d + 1, R.b.shift[0],
                         static_cast<unsigned long long>(stride), novf, static_cast<unsigned long long>(R.buckets()));
    }
    ix->dev.run_rec2[d] = static_cast<const RunRec2 *>(recp);
    ix->runs_report.rec_bytes[d] = R.buckets() * sizeof(RunRec2);
    ix->runs_report.rec_overflow[d] = novf;
    return RBG_OK;
}

// the entries and samples in their final form: at 8-byte positions the low-word pairs and the 6-byte samples, and the lists of P go back
template <typename P>
int pack_depth_final(RunLoad &L, RunDepth &R) {
    rbg_index *ix = L.ix;
    if constexpr (sizeof(P) == 8) {
        void *e2 = nullptr, *s6 = nullptr;
        int rc;
        if ((rc = dev_reserve(ix, (R.E2 + 2) * 8, &e2))) return rc;
        HIP_TRY(static_cast<hipError_t>(launch_pack_pairs32(R.abs_ent, R.E2, 2, e2, nullptr)));
        if (R.abs_samp) {
            if ((rc = dev_reserve(ix, R.E2 * RunsFmt<P>::samp_bytes + 8, &s6))) return rc;
            HIP_TRY(static_cast<hipError_t>(launch_pack_samp48(static_cast<const uint64_t *>(R.abs_samp), R.E2, s6, nullptr)));
        }
        HIP_TRY(hipDeviceSynchronize());
        free_tracked(ix, R.abs_ent);
        if (R.abs_samp) free_tracked(ix, R.abs_samp);
        ix->dev.run_ent2[R.d] = e2;
        ix->dev.run_samp[R.d] = s6;
    } else {
        ix->dev.run_ent2[R.d] = R.abs_ent;
        ix->dev.run_samp[R.d] = R.abs_samp;
    }
    if (L.sw.verbose) {
        size_t f = 0, tt = 0;
        (void)hipMemGetInfo(&f, &tt);
        std::fprintf(stderr, "rbg:   run lists of depth %u in their final form: %llu entries (%llu fillers), directories %.2f GB; HBM in use %.1f GB\n", R.d + 1,
                     static_cast<unsigned long long>(R.E2), static_cast<unsigned long long>(R.fillers), ix->runs_report.dir_bytes[R.d] / 1e9, static_cast<double>(tt - f) / 1e9);
    }
    return RBG_OK;
}

// the depth's DevRunTab2 records and hot words, closed by one more
int append_depth_tables(RunLoad &L, const RunDepth &R) {
    for (size_t t = 0; t < R.nt(); ++t) {
        L.tabs.push_back(DevRunTab2{R.T[t].F, R.first[t], R.b.off[t], R.b.shift[t], 0u});
        if (R.b.off[t] >> kRunHotShiftBit) return RBG_EARG;   // (2^56 buckets: no index that fits a device comes near)
        L.hot.push_back(R.b.off[t] | static_cast<uint64_t>(R.b.shift[t]) << kRunHotShiftBit);
    }
    L.tabs.push_back(DevRunTab2{0, R.E2, 0, 0u, 0u});   // closing record
    L.hot.push_back(0);
    return RBG_OK;
}

// one kept depth: its lists, fillers, folded F, directory or records, final form, table records
template <typename P>
int upload_run_depth(RunLoad &L, uint32_t d, const std::vector<SymTable> &T) {
    RunDepth R(d, T);
    L.ix->dev.run_rec2[d] = nullptr;
    int rc;
    if ((rc = depth_lists_on_device<P>(L, R))) return rc;
    if ((rc = depth_fillers<P>(L, R))) return rc;
    if ((rc = fold_F<P>(L, R))) return rc;
    if ((rc = L.rec_per[d] > 0 ? build_depth_records<P>(L, R) : build_depth_directory<P>(L, R))) return rc;
    if ((rc = pack_depth_final<P>(L, R))) return rc;
    return append_depth_tables(L, R);
}

// the table index: syms, run_tabs2, run_hot and the scalar fields of the layout
int upload_table_index(RunLoad &L) {
    rbg_index *ix = L.ix;
    HostIndex &h = L.h;
    const uint32_t D = L.D;
    for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxKmerDepth); ++d) release_kmer_level(ix, d);   // (levels beyond D, or left over: nothing points at them)
    for (uint32_t d = D; d <= static_cast<uint32_t>(kMaxRunDepth); ++d) ix->dev.run_tab_first[d] = static_cast<uint32_t>(L.tabs.size());
    if (ix->dev.run_tab_first[std::min<uint32_t>(D, kLdsRunDepth)] > static_cast<uint32_t>(kMaxLdsRunTabs)) return RBG_EARG;
    const void *p = nullptr;
    int rc;
    std::vector<DevSym> syms(h.sym.size());   // (no kernel reads a symbol record on this format: F only, for rbg_get_f-style readers)
    for (size_t t = 0; t < syms.size(); ++t) { syms[t] = DevSym{}; syms[t].F = h.sym[t].F; syms[t].nruns = static_cast<uint32_t>(std::min<uint64_t>(h.sym[t].nruns, 0xFFFFFFFFull)); }
    if ((rc = dev_upload(ix, syms.data(), syms.size() * sizeof(DevSym), &p))) return rc;
    ix->dev.syms = static_cast<const DevSym *>(p);
    if ((rc = dev_upload(ix, L.tabs.data(), L.tabs.size() * sizeof(DevRunTab2), &p))) return rc;
    ix->dev.run_tabs2 = static_cast<const DevRunTab2 *>(p);
    if ((rc = dev_upload(ix, L.hot.data(), L.hot.size() * 8, &p))) return rc;
    ix->dev.run_hot = static_cast<const uint64_t *>(p);
    ix->dev.run_ntabs = static_cast<uint32_t>(L.tabs.size());
    ix->dev.run_ksteps = D;
    ix->dev.run_depth_mask = L.mask;
    ix->run_depth_mask = L.mask;
    ix->runs_report.depth_mask_kept = L.mask;
    bool all_recs = true;
    for (uint32_t d = 0; d < D; ++d)
        if (L.mask >> d & 1u) all_recs = all_recs && L.rec_per[d] > 0;
    ix->runs_report.rank_dirs = all_recs ? 0 : 1;   // (1: some kept depth answers its ranks through a directory)
    ix->dev.layout = RBG_LAYOUT_RUNS;
    ix->dev.kmer_steps = 1;
    ix->dev.nmajor = 0;
    if (h.nmajor >= 2) {  // the ftab's word index and the k-mer table index need the major alphabet
        if ((rc = dev_upload(ix, h.major_of, 256, &p))) return rc;
        ix->dev.lut2 = static_cast<const uint8_t *>(p);
        ix->dev.nmajor = h.nmajor;
    }
    return RBG_OK;
}

// the register tables of the in-kernel read staging (rbg_dev.h stage_*; rbg_load_plan.hpp stage_tables)
void set_stage_tables(RunLoad &L) {
    DevIndex &dev = L.ix->dev;
    dev.stage_ok = 0;
    if (L.h.nmajor != 4) return;
    const StageTables s = stage_tables(L.h.major_byte);
    if (!s.ok) return;
    dev.stage_ok = 1;
    dev.stage_shift = s.shift;
    std::memcpy(dev.stage_code, s.code, 8);
    std::memcpy(dev.stage_byte, s.byte, 8);
}

// PHI SLOTS (rbg_load_plan.hpp phi_slot_geometry, phi_by_slots): the slot layout's direct-addressed phi records (rbg_dev.h PhiSlot) answer a phi step from ONE
// sector where the list takes two (directory, entries); at pangenome scale K3 is bound by exactly that sector count.  Cost: about 54 bytes per run at
// 8-byte positions against 16.
template <typename P>
int upload_phi_slots(RunLoad &L, const PhiSlotGeometry &g) {
    rbg_index *ix = L.ix;
    HostIndex &h = L.h;
    rbg_index::RunsReport &rep = ix->runs_report;
    VStage vs("phi slots of the run-indexed layout", true, L.sw.verbose);
    HostBuf<PhiEnt<P>> pe(h.r + 1);
    parallel_for(h.r, [&](uint64_t a, uint64_t b, unsigned) {
        for (uint64_t j = a; j < b; ++j) { pe[j].pos = static_cast<P>(h.pred_pos[j]); pe[j].base = static_cast<P>(h.phi_base[j]); }
    });
    pe[h.r].pos = static_cast<P>(h.n); pe[h.r].base = 0;
    int rc;
    if ((rc = dev_upload(ix, pe.data(), (h.r + 1) * sizeof(PhiEnt<P>), &ix->dev.phi_ent))) return rc;
    const uint64_t nb = g.buckets;
    void *slots = nullptr, *ord = nullptr;
    if ((rc = dev_reserve(ix, nb * g.slot_bytes(), &slots)) || (rc = dev_reserve(ix, nb * sizeof(uint32_t), &ord))) return rc;
    TmpDev ovf;
    if ((rc = ovf.alloc(8))) return rc;
    HIP_TRY(hipMemset(ovf.p, 0, 8));
    ix->dev.phi_packed = g.packed ? 1 : 0;
    ix->dev.phi_shift = g.shift;
    if (launch_build_phi_slots(sizeof(P), g.packed, ix->dev.phi_ent, h.r, h.n, g.shift, slots, static_cast<uint32_t *>(ord), ovf.as<unsigned long long>(), nullptr))
        return RBG_ENODEV;
    unsigned long long novf = 0;
    HIP_TRY(hipMemcpy(&novf, ovf.p, 8, hipMemcpyDeviceToHost));
    ix->phi_slots = nb;
    ix->phi_slots_overflow = novf;
    ix->dev.phi_slots = slots;
    ix->dev.phi_ord = static_cast<const uint32_t *>(ord);
    ix->dev.phi_m = h.r;
    ix->dev.phi_last_pos = h.pred_pos[h.r - 1];
    ix->dev.phi_last_base = h.phi_base[h.r - 1];
    rep.phi_entries = h.r; rep.phi_dir = 0; rep.phi_dir_shift = g.shift; rep.phi_slots = nb; rep.phi_slot_bytes = nb * g.bucket_bytes;
    return RBG_OK;
}

// the phi list at 8-byte positions: fillers, 12-byte entries of low words, the directory with 64-bit super counts under its 32-bit ones
int upload_phi_list_wide(RunLoad &L, uint32_t ds, uint64_t nd, void *dirp, uint64_t *m2, uint64_t *fillers) {
    rbg_index *ix = L.ix;
    HostIndex &h = L.h;
    HostBuf<uint64_t> pe((h.r + 1) * 2);
    parallel_for(h.r, [&](uint64_t a, uint64_t b, unsigned) {
        for (uint64_t j = a; j < b; ++j) { pe[2 * j] = h.pred_pos[j]; pe[2 * j + 1] = h.phi_base[j]; }
    });
    pe[2 * h.r] = h.n; pe[2 * h.r + 1] = 0;   // sentinel: never below a query
    void *abs = nullptr, *none = nullptr;
    HIP_TRY(hipMalloc(&abs, (h.r + 1 + 2) * 16));
    int rc;
    if ((rc = h2d_big(abs, pe.data(), (h.r + 1) * 16))) { (void)hipFree(abs); return rc; }
    uint64_t m_all = h.r + 1;
    std::vector<uint64_t> at;
    rc = add_fillers(ix, true, &abs, &none, false, &m_all, h.n, at, fillers);
    if (rc) { (void)hipFree(abs); return rc; }
    *m2 = m_all - 1;
    void *e12 = nullptr, *sup = nullptr;
    const uint64_t nsup = (nd >> L.sw.super_shift) + 2;
    rc = dev_reserve(ix, (*m2 + 1 + 3) * sizeof(PhiEnt12), &e12);
    if (!rc) rc = dev_reserve(ix, nsup * 8, &sup);
    hipError_t e = hipSuccess;
    if (!rc) e = static_cast<hipError_t>(launch_pack_phi12(abs, *m2 + 1, 3, e12, nullptr));
    if (!rc && e == hipSuccess) e = static_cast<hipError_t>(launch_phi_dir(8, abs, *m2, ds, nd, static_cast<uint32_t *>(dirp), L.sw.super_shift, static_cast<uint64_t *>(sup), nullptr));
    if (!rc && e == hipSuccess) e = hipDeviceSynchronize();
    (void)hipFree(abs);
    if (rc) return rc;
    HIP_TRY(e);
    ix->dev.phi_ent = e12;
    ix->dev.phi_super = static_cast<const uint64_t *>(sup);
    ix->dev.phi_super_shift = L.sw.super_shift;
    return RBG_OK;
}

// the phi list at 4-byte positions: the host's entries as they are, and the directory
int upload_phi_list_narrow(RunLoad &L, uint32_t ds, uint64_t nd, void *dirp) {
    rbg_index *ix = L.ix;
    HostIndex &h = L.h;
    typedef PhiFmt<uint32_t> Fmt;
    HostBuf<unsigned char> pe((h.r + 1 + Fmt::spare) * Fmt::ent_bytes);
    parallel_for(h.r, [&](uint64_t a, uint64_t b, unsigned) {
        for (uint64_t j = a; j < b; ++j) Fmt::put_ent(pe.data(), j, h.pred_pos[j], h.phi_base[j]);
    });
    for (size_t x = 0; x <= Fmt::spare; ++x) Fmt::put_ent(pe.data(), h.r + x, h.n, 0);
    if (const int rc = dev_upload(ix, pe.data(), pe.size(), &ix->dev.phi_ent)) return rc;
    HIP_TRY(static_cast<hipError_t>(launch_phi_dir(4, ix->dev.phi_ent, h.r, ds, nd, static_cast<uint32_t *>(dirp), 0, nullptr, nullptr)));
    HIP_TRY(hipDeviceSynchronize());
    return RBG_OK;
}

// phi over the list of sampled positions and its directory (rbg_load_plan.hpp phi_dir_shift)
template <typename P>
int upload_phi_list(RunLoad &L) {
    rbg_index *ix = L.ix;
    HostIndex &h = L.h;
    rbg_index::RunsReport &rep = ix->runs_report;
    const uint32_t ds = phi_dir_shift(h.r, h.n, L.sw.phi_per, L.max_shift);
    const uint64_t nd = (h.n >> ds) + 2;
    void *dirp = nullptr;
    int rc;
    if ((rc = dev_reserve(ix, nd * 4 + 16, &dirp))) return rc;
    uint64_t m2 = h.r, fillers = 0;
    if constexpr (sizeof(P) == 8) rc = upload_phi_list_wide(L, ds, nd, dirp, &m2, &fillers);
    else rc = upload_phi_list_narrow(L, ds, nd, dirp);
    if (rc) return rc;
    ix->dev.phi_dir = static_cast<const uint32_t *>(dirp);
    ix->dev.phi_dir_shift = ds;
    ix->dev.phi_m = m2;
    ix->dev.phi_last_pos = h.pred_pos[h.r - 1];
    ix->dev.phi_last_base = h.phi_base[h.r - 1];
    rep.phi_entries = m2; rep.phi_fillers = fillers; rep.phi_dir_bytes = nd * 4; rep.phi_dir_shift = ds; rep.phi_dir = 1;
    return RBG_OK;
}

// phi as slots, or as list + directory
template <typename P>
int upload_phi(RunLoad &L) {
    rbg_index *ix = L.ix;
    ix->dev.phi_slots = nullptr;
    ix->dev.phi_ord = nullptr;
    ix->dev.phi_dir = nullptr;
    ix->dev.phi_super = nullptr;
    ix->dev.phi_super_shift = 0;
    if (!L.h.has_tsa) return RBG_OK;
    const PhiSlotGeometry g = phi_slot_geometry(L.h.n, L.h.r, L.h.phi_shift, sizeof(P), L.consts);
    return phi_by_slots(g_opt_run_phi.load(), g, L.h.r, ix->hbm_bytes, ix->hbm_budget) ? upload_phi_slots<P>(L, g) : upload_phi_list<P>(L);
}

template <typename P>
int upload_tables_runs2(rbg_index *ix) {
    RunLoad L(ix, sizeof(P) == 8);   // (reads the switches)
    ix->runs_report.fmt = 2;
    release_slot_lists(ix);
    const std::vector<SymTable> *depth[kMaxRunDepth];
    settle_depths(L, depth);
    ix->dev.run_uni_depth = static_cast<uint32_t>(kMaxRunDepth);   // (no uniform depth, until build_depth_records makes one)
    ix->dev.run_uni_stride = ix->dev.run_uni_shift = 0;
    int rc;
    for (uint32_t d = 0; d < L.D; ++d) {
        ix->dev.run_tab_first[d] = static_cast<uint32_t>(L.tabs.size());
        ix->dev.run_samp[d] = nullptr;
        ix->dev.run_ent2[d] = nullptr; ix->dev.run_dir2[d] = nullptr;
        if (!(L.mask >> d & 1u)) leave_depth_out(L, d);
        else if ((rc = upload_run_depth<P>(L, d, *depth[d]))) return rc;
    }
    if ((rc = upload_table_index(L))) return rc;
    set_stage_tables(L);
    if ((rc = upload_phi<P>(L))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    return RBG_OK;
}

// One marker table on the device: its four arrays, the bucket directory and the bucket records.  Built twice: the SA-row table (DevIndex::mk_*, from the index
// files or rbg_set_markers) and the table keyed by text position (DevIndex::tmk_*, rbg_set_text_markers / .midx) -- the same code under the same gates.
struct DevMarkerTable {
    const uint64_t *start = nullptr, *end = nullptr, *off = nullptr, *vals = nullptr;
    uint64_t nruns = 0;
    const uint32_t *bucket = nullptr;
    uint32_t shift = 0;
    const MkRec *rec = nullptr;
};
// own != nullptr: every array is an allocation of its own (tracked like any other: replicas copy it, rbg_info counts it) and is listed there, so that the
// table can be given back when another one replaces it; else the arrays come from the arena while it has room
int upload_marker_table(rbg_index *ix, const RawMarkers &m, DevMarkerTable &t, std::vector<void *> *own = nullptr) {
    auto up = [&](const void *src, size_t bytes, const void **dst) -> int {
        if (!own) return dev_upload(ix, src, bytes, dst);
        void *p = nullptr;
        const size_t alloc = arena_round(bytes);
        HIP_TRY(hipMalloc(&p, alloc));
        ix->allocs.push_back({p, alloc});
        ix->hbm_bytes += alloc;
        own->push_back(p);
        if (bytes) { const int rc = h2d_big(p, src, bytes); if (rc) return rc; }
        *dst = p;
        return RBG_OK;
    };
    t = DevMarkerTable();
    const void *p = nullptr;
    int rc;
    if ((rc = up(m.start.data(), m.start.size() * 8, &p))) return rc;
    t.start = static_cast<const uint64_t *>(p);
    if ((rc = up(m.end.data(), m.end.size() * 8, &p))) return rc;
    t.end = static_cast<const uint64_t *>(p);
    if ((rc = up(m.off.data(), m.off.size() * 8, &p))) return rc;
    t.off = static_cast<const uint64_t *>(p);
    if ((rc = up(m.vals.data(), m.vals.size() * 8, &p))) return rc;
    t.vals = static_cast<const uint64_t *>(p);
    t.nruns = m.start.size();
    const uint64_t nruns = m.start.size(), n = ix->H().n;
    if (nruns && nruns < 0xFFFFFFFFull) {
        // the shift, the directory, the records and the gates they are built under: rbg_mkdir.hpp
        const uint32_t shift = mk_dir_shift(n, nruns);
        const uint64_t nb = mk_dir_buckets(n, shift);
        std::vector<uint32_t> bucket;
        mk_build_dir(m.end.data(), nruns, n, shift, bucket);
        if ((rc = up(bucket.data(), nb * 4, &p))) return rc;
        t.bucket = static_cast<const uint32_t *>(p);
        t.shift = shift;
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (mk_rec_wanted(shift, std::getenv("RBG_MK_REC"), m.vals.size(), nb, free_b)) {
            std::vector<MkRec> recs;
            mk_build_recs(m.start.data(), m.end.data(), m.off.data(), nruns, m.vals.size(), shift, bucket, recs);
            if ((rc = up(recs.data(), nb * sizeof(MkRec), &p))) return rc;
            t.rec = static_cast<const MkRec *>(p);
        }
    }
    return RBG_OK;
}

int upload_markers(rbg_index *ix) {
    DevIndex &d = ix->dev;
    d.mk_start = d.mk_end = d.mk_off = d.mk_vals = nullptr;
    d.mk_nruns = 0; d.mk_bucket = nullptr; d.mk_shift = 0; d.mk_rec = nullptr;
    DevMarkerTable t;
    const int rc = upload_marker_table(ix, ix->H().ma, t);
    // (as before: what was uploaded before an error stays named in the index)
    d.mk_start = t.start; d.mk_end = t.end; d.mk_off = t.off; d.mk_vals = t.vals; d.mk_nruns = t.nruns;
    d.mk_bucket = t.bucket; d.mk_shift = t.shift; d.mk_rec = t.rec;
    return rc;
}

// the text-position table: replaces the one before it (whose allocations go back first), own allocations throughout
int upload_text_markers(rbg_index *ix, const RawMarkers &m) {
    DevIndex &d = ix->dev;
    HIP_TRY(hipDeviceSynchronize());   // nothing may still read the table that goes
    d.tmk_start = d.tmk_end = d.tmk_off = d.tmk_vals = nullptr;
    d.tmk_nruns = 0; d.tmk_bucket = nullptr; d.tmk_shift = 0; d.tmk_rec = nullptr;
    ix->has_tmk = false;
    for (void *p : ix->tmk_allocs) free_tracked(ix, p);
    ix->tmk_allocs.clear();
    DevMarkerTable t;
    const int rc = upload_marker_table(ix, m, t, &ix->tmk_allocs);
    if (rc) {
        for (void *p : ix->tmk_allocs) free_tracked(ix, p);
        ix->tmk_allocs.clear();
        return rc;
    }
    d.tmk_start = t.start; d.tmk_end = t.end; d.tmk_off = t.off; d.tmk_vals = t.vals; d.tmk_nruns = t.nruns;
    d.tmk_bucket = t.bucket; d.tmk_shift = t.shift; d.tmk_rec = t.rec;
    ix->has_tmk = true;
    return RBG_OK;
}

FlattenOptions current_options();

// give back the device arrays of the k-mer level `depth` (2..5) -- a level the budget rule drops, or one the run-indexed
// layout has copied out
void release_kmer_level(rbg_index *ix, uint32_t depth) {
    if (depth < 2 || depth - 2 >= ix->kmer_levels.size()) return;
    ComposedLevel &L = ix->kmer_levels[depth - 2];
    for (void *p : {L.ent, L.samp}) {
        if (!p) continue;
        for (size_t i = 0; i < ix->allocs.size(); ++i)
            if (ix->allocs[i].p == p) { ix->hbm_bytes -= ix->allocs[i].bytes; ix->allocs.erase(ix->allocs.begin() + static_cast<std::ptrdiff_t>(i)); break; }
        (void)hipFree(p);
    }
    L = ComposedLevel();
}
std::vector<SymTable> &kmer_level_tables(HostIndex &h, uint32_t depth) { return h.kmer(depth); }
uint32_t depth_of_level(const HostIndex &h, const std::vector<SymTable> *lvl) { return static_cast<uint32_t>(lvl - h.kmer_lv) + 2u; }
void drop_kmer_level(rbg_index *ix, std::vector<SymTable> &lvl) {
    release_kmer_level(ix, depth_of_level(ix->H(), &lvl));
    std::vector<SymTable>().swap(lvl);
}

// Depths 2 .. kmer_deferred composed on the device (k_compose.hip) from the depth-1 tables of the k-mer alphabet and the
// BWT's own runs; the host tables get their metadata (runs, total, F, bucket shift) and pointers into the level arrays.
// Without the memory for it (or with RBG_HOST_COMPOSE=1 at flatten time) the host composes as before.
template <typename P> int compose_on_device_k(rbg_index *ix, uint32_t K);

// Depths 2 .. kmer_deferred on the device; when neither the device (transient HBM: about 100 bytes per piece of the deepest
// intermediate depth) nor the host (24 bytes per run and depth, refused when the container's memory would not hold it) can
// compose that many symbols per step, one symbol less is tried -- said on stderr, and rbg_info reports the depth asked for beside
// the depth kept.  (Round 4: an r = 1e9 index gets 3 symbols per step this way where 5 would need more than the device has.)
template <typename P>
int compose_on_device(rbg_index *ix) {
    HostIndex &h = ix->H();
    const uint32_t M = h.nmajor, K0 = h.kmer_deferred;
    h.kmer_deferred = 0;
    if (M < 1 || K0 < 2) return RBG_OK;
    if (ix->kmer_steps_requested == 0) ix->kmer_steps_requested = K0;
    // How deep is worth composing is decided BEFORE composing (planned_depth): a depth takes minutes and hundreds of GB of transient HBM at r = 1e9,
    // and one the budget rule of upload() then drops -- or whose composition fails after the shallower ones were made -- was composed for nothing.
    // The fallback below still catches an estimate that was too kind.
    uint32_t K_plan = K0;
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            free_b = assumed_free_hbm(free_b, assumed_free_env().mb);
            const double budget = static_cast<double>(load_budget(free_b, g_opt_hbm_budget_mb.load(), ix->plan_budget));
            K_plan = planned_depth(static_cast<double>(h.r), h.has_tsa, K0, static_cast<double>(free_b), budget, runs_certain(g_opt_rank_layout.load(), ix->auto_runs));
            if (K_plan < K0)
                std::fprintf(stderr, "rbg: r = %.3g runs, %.1f GB free, %.1f GB replica budget: composing %u symbol(s) per step, not the %u asked for (estimated: depth %u would "
                                     "hold about %.3g runs; RBG_OPT_HBM_BUDGET_MB / RBG_OPT_RUN_DEPTHS change what fits)\n", static_cast<double>(h.r), free_b / 1e9, budget / 1e9,
                             K_plan, K0, K0, est_depth_runs(static_cast<double>(h.r), K0));
        }
    }
    if (K_plan < 2) return RBG_OK;   // single-symbol steps: nothing to compose
    for (uint32_t K = K_plan; K >= 2; --K) {
        // (a pass that failed partway -- the host fallback included -- must leave nothing of a deeper level behind: levels() and
        //  level_has_data() count what they find)
        for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxKmerDepth); ++d) { release_kmer_level(ix, d); std::vector<SymTable>().swap(kmer_level_tables(h, d)); }
        ix->kmer_levels.clear();
        ix->runs_forced = false;
        const int rc = compose_on_device_k<P>(ix, K);
        if (rc != RBG_ENOMEM) return rc;
        std::fprintf(stderr, "rbg: %u symbols per step cannot be composed in the memory there is: trying %u\n", K, K - 1);
        (void)hipGetLastError();
    }
    return RBG_OK;   // single-symbol steps: nothing to compose
}

template <typename P>
int compose_on_device_k(rbg_index *ix, const uint32_t K) {
    HostIndex &h = ix->H();
    const uint32_t M = h.nmajor;
    const FlattenOptions opt = current_options();
    const auto t0 = std::chrono::steady_clock::now();
    struct Hold {
        std::vector<void *> p;
        ~Hold() { for (void *q : p) if (q) (void)hipFree(q); }
        int put(const void *src, size_t bytes, void **out) {
            void *d = nullptr;
            hipError_t e = hipMalloc(&d, bytes ? bytes : 16);
            if (e != hipSuccess) { (void)hipGetLastError(); return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV; }
            p.push_back(d);
            if (bytes && h2d_big(d, src, bytes) != RBG_OK) return RBG_ENODEV;
            *out = d;
            return RBG_OK;
        }
    } hold;
    int rc = RBG_OK;
    ComposeTable major[4];
    for (uint32_t m = 0; m < M && !rc; ++m) {
        const SymTable &t = h.sym[h.major_slot[m]];
        PreparedSym<P> ps;
        prepare_sym<P>(t, h.has_tsa, ps);
        void *de = nullptr, *dsp = nullptr;
        rc = hold.put(ps.ent.data(), ps.ent.size() * sizeof(RunEnt<P>), &de);
        if (!rc && h.has_tsa) rc = hold.put(ps.samp.data(), ps.samp.size() * sizeof(P), &dsp);
        major[m] = ComposeTable{de, dsp, t.nruns, t.total, t.F};
    }
    void *g_start = nullptr, *g_id = nullptr, *g_samp = nullptr;
    if (!rc) {   // depth 1: the BWT runs themselves, id = major index of the head, sample = samples_last_ (SA - 1)
        HostBuf<P> gs(h.r + 1), sp(h.has_tsa ? h.r : 0);
        HostBuf<uint32_t> gi(h.r);
        gs[h.r] = static_cast<P>(h.run_start[h.r]);
        parallel_for(h.r, [&](uint64_t b, uint64_t e, unsigned) {
            for (uint64_t g = b; g < e; ++g) {
                gs[g] = static_cast<P>(h.run_start[g]);
                const uint8_t m = h.major_of[h.run_heads[g]];
                gi[g] = m == 0xFF ? 0xFFFFFFFFu : m;
                if (h.has_tsa) sp[g] = static_cast<P>(h.samples_last[g]);
            }
        });
        rc = hold.put(gs.data(), gs.size() * sizeof(P), &g_start);
        if (!rc) rc = hold.put(gi.data(), gi.size() * 4, &g_id);
        if (!rc && h.has_tsa) rc = hold.put(sp.data(), sp.size() * sizeof(P), &g_samp);
    }
    if (std::getenv("RBG_VERBOSE"))
        std::fprintf(stderr, "rbg:   compose: depth-1 tables and runs converted and copied in %.2f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    std::vector<ComposedLevel> levels;
    // When the run-indexed layout is certain (asked for, or not even the single-symbol slot tables fit the budget: the test
    // options_for makes) the depths its depth set leaves out give their arrays back as soon as the next depth is made.
    uint32_t keep_mask = 0;
    {
        bool certain = runs_certain(g_opt_rank_layout.load(), ix->auto_runs);
        if (!certain && layout_automatic()) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
                // THIS budget differs from the load's (upload(), options_for(), compose_on_device above): the free memory as it is now, no budget planned
                // before the load and no RBG_ASSUME_FREE_HBM_MB cap.  Whether it should is undecided; the rules were moved, not changed.
                certain = slot_level1_estimate(h.n, h.sigma, sizeof(P), load_consts()) > static_cast<double>(load_budget(free_b, g_opt_hbm_budget_mb.load(), /*plan_budget=*/0));
        }
        if (certain && h.sigma <= static_cast<uint32_t>(kLdsSyms)) keep_mask = asked_depth_mask(g_opt_run_depths.load(), K) | 1u << (K - 1);
    }
    // (with the run-indexed layout certain, the composition also frees its inputs as soon as they have been read: nothing
    //  after it needs the depth-1 lists in this form -- upload_tables_runs2 builds depth 1 from the host tables)
    bool released[2] = {false, false};
    if (!rc) rc = compose_levels_device(sizeof(P), h.n, M, major, g_start, static_cast<const uint32_t *>(g_id), g_samp, h.r, K, h.has_tsa, levels, nullptr, keep_mask,
                                        keep_mask ? released : nullptr);
    if (released[0])
        for (void *&held : hold.p)
            if (held == g_start || held == g_id || held == g_samp) held = nullptr;
    if (released[1])
        for (uint32_t m = 0; m < M; ++m) {
            for (void *&held : hold.p)
                if (held == major[m].ent || held == major[m].samp) held = nullptr;
            major[m].ent = major[m].samp = nullptr;
        }
    if (rc == RBG_EARG) {   // 2^32 pieces in one depth (r beyond about 1.7e9 at five symbols): the device sweeps index pieces with 32 bits, the host composition does not
        std::fprintf(stderr, "rbg: a k-mer depth has 2^32 pieces or more: the device composition indexes them with 32 bits\n");
        rc = RBG_ENOMEM;
    }
    if (rc == RBG_ENOMEM || rc == RBG_ENODEV) {   // not enough HBM for the sweeps' temporaries: the host composes instead
        for (ComposedLevel &L : levels) { if (L.ent) (void)hipFree(L.ent); if (L.samp) (void)hipFree(L.samp); }
        (void)hipGetLastError();
        // the host composition holds every depth as three 8-byte vectors per run: 24 bytes x (about 1.6 + 2.1 + 2.6 + 3.2) runs of the
        // BWT at pangenome scale -- it must not be what exhausts the machine (a container's memory limit kills the process, and on a
        // shared box more than that)
        const double need_host = 24.0 * 3.3 * static_cast<double>(K - 1) * static_cast<double>(h.r);
        const double have_host = host_memory_available();
        if (need_host > 0.8 * have_host) {
            std::fprintf(stderr, "rbg: composing the k-mer tables on the device failed (%s), and the host composition would need about %.0f GB of the %.0f GB "
                                 "this process may still use: not attempted (fewer symbols per step -- RBG_OPT_KMER_STEPS -- need less of both)\n",
                         rbg_strerror(rc), need_host / 1e9, have_host / 1e9);
            return RBG_ENOMEM;
        }
        std::fprintf(stderr, "rbg: composing the k-mer tables on the device failed (%s): composing on the host\n", rbg_strerror(rc));
        return compose_kmer_tables_host(h, static_cast<int>(K), opt);
    }
    if (rc) {
        for (ComposedLevel &L : levels) { if (L.ent) (void)hipFree(L.ent); if (L.samp) (void)hipFree(L.samp); }
        return rc;
    }
    ix->kmer_levels = std::move(levels);
    ix->runs_forced = keep_mask != 0;
    // the depth-1 run lists of the k-mer alphabet are on the device in the very form the slot tables are built from
    // (commit_sym): they stay, instead of being converted and copied a second time (5 + 2.5 GB at r = 3e8)
    for (uint32_t m = 0; m < M && !released[1]; ++m) {
        SymTable &t = h.sym[h.major_slot[m]];
        for (void *q : {const_cast<void *>(major[m].ent), const_cast<void *>(major[m].samp)}) {
            if (!q) continue;
            for (void *&held : hold.p)
                if (held == q) held = nullptr;
            const size_t bytes = q == major[m].ent ? (t.nruns + 1) * sizeof(RunEnt<P>) : std::max<size_t>(16, t.nruns * sizeof(P));
            ix->allocs.push_back({q, bytes});
            ix->hbm_bytes += bytes;
        }
        t.dev_ent = major[m].ent;
        t.dev_samp = major[m].samp;
    }
    for (uint32_t d = 2; d <= K; ++d) {
        ComposedLevel &L = ix->kmer_levels[d - 2];
        if (L.ent) {   // (a depth outside the run-indexed layout's depth set has given its arrays back already: metadata only)
            ix->allocs.push_back({L.ent, (L.entries + 2) * sizeof(RunEnt<P>)});
            ix->hbm_bytes += (L.entries + 2) * sizeof(RunEnt<P>);
        }
        if (L.samp) { ix->allocs.push_back({L.samp, (L.entries + 2) * sizeof(P)}); ix->hbm_bytes += (L.entries + 2) * sizeof(P); }
        std::vector<SymTable> &tabs = kmer_level_tables(h, d);
        tabs.assign(L.nruns.size(), SymTable());
        for (size_t t = 0; t < tabs.size(); ++t) {
            SymTable &st = tabs[t];
            st.byte = h.major_byte[t % M];
            st.nruns = L.nruns[t];
            st.total = L.total[t];
            st.F = L.F[t];
            st.shift = kmer_table_shift(h.n, st.nruns, d, opt);
            if (st.shift > 12 || (st.shift > 8 && (h.n >> 40))) return RBG_EARG;  // wide buckets carry 40-bit ranks (rbg_dev.h)
            if (st.nruns >= 0xFFFFFFF0ull) return RBG_EARG;
            st.dev_ent = L.ent ? static_cast<const char *>(L.ent) + L.first[t] * sizeof(RunEnt<P>) : nullptr;
            st.dev_samp = L.samp ? static_cast<const char *>(L.samp) + L.first[t] * sizeof(P) : nullptr;
        }
    }
    if (std::getenv("RBG_VERBOSE"))
        std::fprintf(stderr, "rbg: k-mer tables composed on the device %.2f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return RBG_OK;
}

// does k-mer depth d (2..5) still have its run lists -- on the host, or composed on the device and not given back?
bool level_has_data(const rbg_index *ix, uint32_t d) {
    const std::vector<SymTable> &T = ix->H().kmer(d);
    if (T.empty()) return false;
    if (d - 2 < ix->kmer_levels.size() && ix->kmer_levels[d - 2].ent) return true;
    for (const SymTable &t : T)
        if (t.start.size() == t.nruns + 1) return true;
    return false;
}

bool compose_deferred(int device);
inline int levels_of(const HostIndex &h) { return static_cast<int>(h.kmer_levels()); }

}  // namespace
