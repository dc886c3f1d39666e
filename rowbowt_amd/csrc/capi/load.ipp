// capi/load.ipp -- upload() and options_for() as sequences of named steps (their rules: rbg_load_plan.hpp), finish(); the loading / converting / building
// entry points, rbg_info and the host-array accessors.  (What the query entry points share -- ReadBatch, the result pool, d2h_result -- is query.ipp.)
// Part of rbg_capi.hip.
namespace {
// What the steps of upload() hand to each other beside the index itself.
struct LoadPlan {
    int compute_units = 0;
    size_t free_b = 0, budget = 0;   // free HBM and replica budget of this load (as options_for() saw them, where it looked)
    bool runs_layout = false;
};

int compose_both_widths(rbg_index *ix) { return ix->H().pos_bytes == 4 ? compose_on_device<uint32_t>(ix) : compose_on_device<uint64_t>(ix); }
size_t slot_need(const HostIndex &h) { return h.pos_bytes == 4 ? replica_bytes<uint32_t>(h) : replica_bytes<uint64_t>(h); }
size_t runs_need(const HostIndex &h, uint32_t mask) { return runs_replica_bytes(shape_of(h), load_consts(), mask); }

int check_device(const rbg_index *ix, LoadPlan &p) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ix->device < 0 || ix->device >= ndev) {
        std::fprintf(stderr, "rbg: no usable HIP device %d (found %d); this library has no CPU path\n", ix->device, ndev);
        return RBG_ENODEV;
    }
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, ix->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::fprintf(stderr, "rbg: device %d is %s; kernels are built for gfx950 (MI355X) only\n", ix->device, prop.gcnArchName);
        return RBG_ENODEV;
    }
    p.compute_units = prop.multiProcessorCount;
    return RBG_OK;
}

// the device's description of the index, and the k-mer depths where flatten() left them to the device
int compose_if_deferred(rbg_index *ix) {
    HostIndex &h = ix->H();
    DevIndex &d = ix->dev;
    d = DevIndex{};
    d.n = h.n;
    d.r = h.r;
    d.sigma = h.sigma;
    d.pos_bytes = h.pos_bytes;
    d.has_tsa = h.has_tsa ? 1 : 0;
    d.last_run_sample = h.last_run_sample;
    d.phi_shift = h.phi_shift;
    if (h.kmer_deferred) return compose_both_widths(ix);   // depths 2.. composed on the device (flatten() only chose the k-mer alphabet)
    return RBG_OK;
}

// The k-mer tables buy speed with memory: keep the deepest level that fits a quarter of the free HBM
// (rbg_load_plan.hpp default_budget) or RBG_OPT_HBM_BUDGET_MB.
int fix_budget(rbg_index *ix, LoadPlan &p) {
    size_t total_b = 0;
    HIP_TRY(hipMemGetInfo(&p.free_b, &total_b));
    // (the budget options_for() fixed before the composition put its levels on the device, where it was taken: VERDICT r4 item 8)
    p.budget = load_budget(p.free_b, g_opt_hbm_budget_mb.load(), ix->plan_budget);
    if (ix->plan_free) p.free_b = static_cast<size_t>(ix->plan_free);
    return RBG_OK;
}

// Layout: the slot tables cost n/16 bytes per table + n/2 (n at 8-byte positions) for phi, whatever r is.  When
// even the single-symbol level does not fit the budget -- or on request -- the run-indexed layout takes over
// (space proportional to r; wave-cooperative predecessor search, k_runs.hip).
void decide_layout(rbg_index *ix, LoadPlan &p) {
    HostIndex &h = ix->H();
    p.runs_layout = runs_certain(g_opt_rank_layout.load(), ix->auto_runs);
    if (!p.runs_layout && layout_automatic()) {
        size_t lvl1 = 0;  // the single-symbol level alone
        {
            std::vector<SymTable> held[kMaxKmerDepth - 1];
            for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxKmerDepth); ++d) held[d - 2].swap(h.kmer(d));
            lvl1 = slot_need(h);
            for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxKmerDepth); ++d) held[d - 2].swap(h.kmer(d));
        }
        p.runs_layout = lvl1 > p.budget;
    }
}

// RBG_LAYOUT_AUTO, second look (options_for's was an estimate from n alone, before anything was composed): if the slot tables of the
// levels at hand exceed the budget, the rule below would give the deep levels wider buckets and then drop levels -- the run-indexed
// layout keeps every level at full speed instead, while it fits (about 110 bytes per run at its leanest).  Measured on the bench
// index at the default budget: 1.13e9 reads/s from the 70 GB of five symbols in wide buckets, 1.14e9 from the 59 GB of four
// symbols, 1.23e9 from the 8.7 GB of this layout (profiles/r04_bench.json space_speed / value_library_default).
int second_look_at_layout(rbg_index *ix, LoadPlan &p) {
    HostIndex &h = ix->H();
    if (p.runs_layout || g_opt_rank_layout.load() != RBG_LAYOUT_AUTO || h.kmer(2).empty() || h.sigma > static_cast<uint32_t>(kLdsSyms) ||
        slot_need(h) <= p.budget || !runs_layout_fits(h.r, static_cast<double>(p.budget)))
        return RBG_OK;
    if (std::getenv("RBG_VERBOSE"))
        std::fprintf(stderr, "rbg: device %d: the slot tables of all k-mer levels (%.1f GB) exceed the %.1f GB replica budget: the run-indexed layout instead of "
                             "wider buckets or fewer symbols per step (RBG_LAYOUT_PREFER_SLOTS keeps slot tables)\n", ix->device, slot_need(h) / 1e9, p.budget / 1e9);
    p.runs_layout = true;
    ix->auto_runs = true;
    // the levels at hand are the slot layout's (at most kMaxSlotKmerDepth, composed before this look could be taken); the run-indexed
    // layout steps by as many symbols as were asked for: compose again, that deep (rare: options_for's estimate usually decides first)
    const uint32_t asked = static_cast<uint32_t>(std::min<int64_t>(g_opt_kmer_steps.load(), kMaxKmerDepth));
    if (asked > h.kmer_levels() && compose_deferred(ix->device) && h.nmajor >= 1) {
        for (SymTable &t : h.sym) {
            free_tracked(ix, const_cast<void *>(t.dev_ent));
            free_tracked(ix, const_cast<void *>(t.dev_samp));
            t.dev_ent = t.dev_samp = nullptr;
        }
        h.kmer_deferred = asked;
        ix->kmer_steps_requested = asked;
        return compose_both_widths(ix);
    }
    return RBG_OK;
}

void settle_layout(rbg_index *ix, LoadPlan &p) {
    HostIndex &h = ix->H();
    if (ix->runs_forced) p.runs_layout = true;
    if (p.runs_layout && h.sigma > static_cast<uint32_t>(kLdsSyms)) {
        std::fprintf(stderr, "rbg: %u distinct symbols: the run-indexed layout serves at most %d; keeping the slot tables\n", h.sigma, kLdsSyms);
        p.runs_layout = false;
    }
    ix->runs_layout = p.runs_layout;
    if (!p.runs_layout)   // (the slot layout stages at most kMaxSlotKmerDepth symbols per gather)
        while (levels_of(h) > kMaxSlotKmerDepth) drop_kmer_level(ix, h.kmer(h.kmer_levels()));
}

// one step of what rbg_load_plan.hpp trim_run_depths / trim_to_ends_for_records decided: said, and applied to the index
void apply_trim_step(rbg_index *ix, const TrimStep &s, size_t budget) {
    if (s.kind == TrimStep::kLeaveOutDepth)
        std::fprintf(stderr, "rbg: run-indexed replica of %.1f GB exceeds the %.1f GB budget: leaving out the run lists of depth %u\n", s.need / 1e9, budget / 1e9, s.depth);
    if (s.kind == TrimStep::kDropDeepest)
        std::fprintf(stderr, "rbg: run-indexed replica of %.1f GB exceeds the %.1f GB budget: dropping the %zu-table k-mer level\n", s.need / 1e9, budget / 1e9, s.tables);
    if (s.kind == TrimStep::kEndsOnly)
        std::fprintf(stderr, "rbg: bucket records for every kept depth (%.1f GB with them) exceed the %.1f GB budget: leaving out the depths between 1 and %d "
                             "(%.1f GB with records for both)\n", s.need / 1e9, budget / 1e9, static_cast<int>(s.depth), s.with_ends / 1e9);
    if (s.drops_level()) drop_kmer_level(ix, ix->H().kmer(s.depth));
}

// Run-indexed layout: the k-mer depths stay (their run lists are O(r) too: DevRunTab2, rbg_dev.h); RBG_OPT_RUN_DEPTHS or the default set names those that
// get run lists (default: the deepest, half of it, ... 1 -- 0xFF keeps them all), and over budget depths go in the order of rbg_load_plan.hpp.
void trim_run_levels(rbg_index *ix, const LoadPlan &p) {
    HostIndex &h = ix->H();
    if (ix->kmer_steps_requested == 0) ix->kmer_steps_requested = static_cast<uint64_t>(levels_of(h));
    ix->runs_report = rbg_index::RunsReport();
    ix->runs_report.depth_mask_asked = static_cast<uint32_t>(g_opt_run_depths.load());
    const IndexShape shape = shape_of(h);
    const LoadConsts consts = load_consts();
    const uint32_t levels = h.kmer_levels();
    uint32_t has_data = 1u;
    for (uint32_t d = 2; d <= levels; ++d)
        if (level_has_data(ix, d)) has_data |= 1u << (d - 1);
    RunTrim t = trim_run_depths(shape, consts, asked_depth_mask(g_opt_run_depths.load(), levels), levels, p.budget, has_data);
    if (ends_only_rule_applies(g_opt_run_depths.load(), g_opt_run_rec.load(), t.levels)) {
        const uint32_t max_shift = h.pos_bytes == 8 ? static_cast<uint32_t>(env_opt("RBG_RUN_FILL_SHIFT", kRunFillShift, 4, kRunFillShift)) : 31u;
        trim_to_ends_for_records(shape, consts, t, p.budget, max_shift, g_opt_run_phi.load());
    }
    for (const TrimStep &s : t.steps) apply_trim_step(ix, s, p.budget);
    ix->runs_report.depths_dropped_budget = t.depths_dropped_budget;
    for (uint32_t d = 2; d < t.levels; ++d)   // the depths left out give their device arrays back now
        if (!(t.mask >> (d - 1) & 1u)) {
            release_kmer_level(ix, d);
            for (SymTable &st : kmer_level_tables(h, d)) st.dev_ent = st.dev_samp = nullptr;
        }
    ix->run_depth_mask = t.mask;
}

// Slot layout over budget: first give the k-mer levels wider buckets, deepest level first (their runs are sparse: rbg_load_plan.hpp widened_shift
// -- a few per cent slower per step), then drop the deepest level and try again.  At pangenome scale this keeps a level more than
// dropping alone.
void trim_slot_levels(rbg_index *ix, const LoadPlan &p) {
    HostIndex &h = ix->H();
    const LoadConsts consts = load_consts();
    bool widened = false;
    while (slot_need(h) > p.budget && !h.kmer(2).empty()) {
        if (!widened && g_opt_deep_shift.load() < 0 && g_opt_rank_shift.load() < 0) {
            widened = true;
            for (uint32_t wd = static_cast<uint32_t>(kMaxSlotKmerDepth); wd >= 2; --wd) {
                std::vector<SymTable> &lvl = h.kmer(wd);
                if (lvl.empty() || slot_need(h) <= p.budget) continue;
                const size_t before = slot_need(h);
                for (SymTable &t : lvl) t.shift = widened_shift(h.n, t.nruns, t.shift, consts);
                if (slot_need(h) != before)
                    std::fprintf(stderr, "rbg: replica of %.1f GB exceeds the %.1f GB budget: wider buckets for the %zu-table k-mer level (%.1f GB)\n",
                                 before / 1e9, p.budget / 1e9, lvl.size(), slot_need(h) / 1e9);
            }
            continue;
        }
        std::vector<SymTable> &deepest = h.kmer(h.kmer_levels());
        std::fprintf(stderr, "rbg: replica of %.1f GB exceeds the %.1f GB budget: dropping the %zu-table k-mer level\n",
                     slot_need(h) / 1e9, p.budget / 1e9, deepest.size());
        drop_kmer_level(ix, deepest);
    }
}

void say_what_is_kept(const rbg_index *ix, const LoadPlan &p) {
    const HostIndex &h = ix->H();
    const int levels = levels_of(h);
    // (the slot layout stages at most kMaxSlotKmerDepth symbols per gather: a default request of eight that became five there is not news)
    const uint64_t asked_here = p.runs_layout ? ix->kmer_steps_requested : std::min<uint64_t>(ix->kmer_steps_requested, static_cast<uint64_t>(kMaxSlotKmerDepth));
    if (std::getenv("RBG_VERBOSE") || static_cast<uint64_t>(levels) != asked_here)
        std::fprintf(stderr, "rbg: device %d: %.1f GB free, replica budget %.1f GB: keeping %d of %llu symbol(s) per %s (%.1f GB)\n", ix->device,
                     p.free_b / 1e9, p.budget / 1e9, levels, static_cast<unsigned long long>(ix->kmer_steps_requested), p.runs_layout ? "search step" : "gather",
                     (p.runs_layout ? runs_need(h, ix->run_depth_mask) : slot_need(h)) / 1e9);
    if (p.runs_layout && std::getenv("RBG_VERBOSE")) std::fprintf(stderr, "rbg: device %d: k-mer depths with run lists: mask 0x%x\n", ix->device, ix->run_depth_mask);
}

int upload_layout_tables(rbg_index *ix, const LoadPlan &p) {
    HostIndex &h = ix->H();
    ix->dev.layout = RBG_LAYOUT_SLOTS;
    if (p.runs_layout) {
        if (std::getenv("RBG_VERBOSE")) std::fprintf(stderr, "rbg: device %d: run-indexed layout (space proportional to r)\n", ix->device);
        return h.pos_bytes == 4 ? upload_tables_runs2<uint32_t>(ix) : upload_tables_runs2<uint64_t>(ix);
    }
    ix->arena_bytes = h.pos_bytes == 4 ? replica_bytes<uint32_t>(h, true) : replica_bytes<uint64_t>(h, true);   // (without the lists that are on the device already)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (ix->arena_bytes > free_b) {
        std::fprintf(stderr, "rbg: index needs %.1f GB of HBM, %.1f GB free\n", ix->arena_bytes / 1e9, free_b / 1e9);
        return RBG_ENOMEM;
    }
    {
        VStage vs("arena hipMalloc");
        // (a platform cost: fresh VRAM is mapped and cleared at some 45-70 GB/s when the memory was freed shortly before --
        //  2.7-7 s for the bench replica's 218 GB -- and next to nothing when it has been idle: tools/alloc_probe.py,
        //  profiles/r03_load_time.txt.  Asking for the block from a helper thread while the host flattens and the
        //  device composes was tried: the driver serialises the composition's own allocations behind it, no gain.)
        HIP_TRY(hipMalloc(&ix->arena, ix->arena_bytes));
    }
    ix->allocs.push_back({ix->arena, ix->arena_bytes});
    ix->hbm_bytes += ix->arena_bytes;
    ix->arena_used = 0;
    return h.pos_bytes == 4 ? upload_tables<uint32_t>(ix) : upload_tables<uint64_t>(ix);
}

int upload_small_arrays(rbg_index *ix, const LoadPlan &p) {
    HostIndex &h = ix->H();
    DevIndex &d = ix->dev;
    int rc;
    const void *ptr = nullptr;
    if ((rc = dev_upload(ix, h.lut, 256, &ptr))) return rc;
    d.lut = static_cast<const uint8_t *>(ptr);
    const unsigned long long zero[4] = {0, 0, 0, 0};
    if ((rc = dev_upload(ix, zero, sizeof(zero), &ptr))) return rc;
    d.counters = const_cast<unsigned long long *>(static_cast<const unsigned long long *>(ptr));
    if (h.has_ma) {
        VStage vs("markers");
        if ((rc = upload_markers(ix))) return rc;
    }
    ix->cfg.block_threads = static_cast<int>(g_opt_block_threads.load());
    ix->cfg.max_blocks = p.compute_units * 32;
    return RBG_OK;
}

// ftab (next-row f3): built last, with the finished replica, by searching every word on the GPU
int build_ftab(rbg_index *ix) {
    const HostIndex &h = ix->H();
    DevIndex &d = ix->dev;
    d.ftab = nullptr;
    d.ftab_k = 0;
    int64_t fk = g_opt_ftab_k.load();
    if (fk < 0) fk = auto_ftab_k(d.nmajor, h.n);
    if (fk <= 0 || d.nmajor < 2) return RBG_OK;
    VStage vs("ftab");
    const double words = ftab_words(d.nmajor, fk);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t entry = ftab_entry_bytes(h.pos_bytes);
    if (!ftab_fits(words, entry, words < 4.0e9 ? ftab_build_scratch_bytes(static_cast<uint64_t>(words), static_cast<uint32_t>(fk)) : 0, free_b)) return RBG_OK;
    const uint64_t W = static_cast<uint64_t>(words);
    void *tab = nullptr;
    HIP_TRY(hipMalloc(&tab, W * entry));
    ix->allocs.push_back({tab, static_cast<size_t>(W * entry)});
    ix->hbm_bytes += W * entry;
    if (launch_build_ftab(d, ix->cfg, static_cast<uint32_t>(fk), tab, nullptr)) return RBG_ENODEV;
    d.ftab = tab;
    d.ftab_k = static_cast<uint32_t>(fk);
    HIP_TRY(hipMemset(d.counters, 0, 4 * sizeof(uint64_t)));  // the build's own searches are not user queries
    return RBG_OK;
}

// jump table (rbg_jump.h, k_jump.hip): built after the ftab and after every decision above -- the lowest priority of the budget, so the
// layout is the one the replica has without it (rbg_layout_info identical).  What the budget leaves holds the table or nothing.
int build_jump_table(rbg_index *ix) {
    DevIndex &d = ix->dev;
    d.jump = nullptr;
    d.jump_buckets = 0;
    d.jump_k = 0;
    d.jump2_buckets = 0;
    d.jump2_k = 0;
    d.jump_complete = 0;
    int64_t jk = g_opt_jump_k.load();
    const bool jump_auto = jk < 0;
    if (jump_auto) jk = auto_jump_k(ix->hbm_bytes);
    if (jk <= 0) return RBG_OK;
    // level 2 (rbg_jump.h): only where level 1 is, after it, from what the budget still leaves
    const int64_t jk2 = jump2_k_for(g_opt_jump2_k.load(), jump_auto, jk);
    VStage vs("jump table");
    const auto t0 = std::chrono::steady_clock::now();
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const JumpBudgets jb = jump_budgets(ix->hbm_budget, ix->hbm_bytes, free_b, jump_auto);
    void *tab = nullptr;
    uint64_t bytes = 0, nb = 0, keys = 0, words = 0;
    const char *why = nullptr;
    JumpLevel2 l2;
    int rc = launch_build_jump(d, ix->cfg, static_cast<uint32_t>(jk), jb.table_budget, jb.peak_budget, &tab, &bytes, &nb, &keys, &why, nullptr,
                               static_cast<uint32_t>(jk2), jb.both_budget, &l2, &words);
    if (rc == static_cast<int>(hipErrorOutOfMemory)) { (void)hipGetLastError(); rc = 0; why = "out of device memory while building it"; }
    if (rc) return RBG_ENODEV;
    HIP_TRY(hipMemset(d.counters, 0, 4 * sizeof(uint64_t)));  // (the build's own searches are not user queries)
    ix->jump_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() - l2.build_ms;
    if (tab) {
        ix->allocs.push_back({tab, static_cast<size_t>(bytes + l2.bytes)});   // (level 2 lies behind level 1 in the same array)
        ix->hbm_bytes += bytes + l2.bytes;
        d.jump = tab;
        d.jump_buckets = nb;
        d.jump_k = static_cast<uint32_t>(jk);
        ix->jump_k = static_cast<uint64_t>(jk);
        ix->jump_keys = keys;
        ix->jump_bytes = bytes;
        ix->jump_buckets = nb;
        if (std::getenv("RBG_VERBOSE"))
            std::fprintf(stderr, "rbg: device %d: jump table of %lld-mers: %llu keys, %.2f GB, %.0f ms\n", ix->device, static_cast<long long>(jk),
                         static_cast<unsigned long long>(keys), bytes / 1e9, ix->jump_build_ms);
        if (l2.tab) {
            d.jump2_buckets = l2.buckets;
            d.jump2_k = static_cast<uint32_t>(jk2);
            ix->jump2_k = static_cast<uint64_t>(jk2);
            ix->jump2_keys = l2.keys;
            ix->jump2_bytes = l2.bytes;
            ix->jump2_buckets = l2.buckets;
            ix->jump2_build_ms = l2.build_ms;
            if (std::getenv("RBG_VERBOSE"))
                std::fprintf(stderr, "rbg: device %d: jump table, level 2, of %lld + %lld symbols: %llu keys, %.2f GB, %.0f ms\n", ix->device,
                             static_cast<long long>(jk), static_cast<long long>(jk2), static_cast<unsigned long long>(l2.keys), l2.bytes / 1e9, l2.build_ms);
        } else if (jk2 > 0 && std::getenv("RBG_VERBOSE")) {
            std::fprintf(stderr, "rbg: device %d: no level 2 of the jump table (%lld + %lld symbols; %llu words occur): %s\n", ix->device, static_cast<long long>(jk),
                         static_cast<long long>(jk2), static_cast<unsigned long long>(l2.keys), l2.why ? l2.why : "skipped");
        }
        // the levels whose absent keys end a read at the probe (rbg_jump.h jump_complete_mask).  RBG_JUMP_ABSENT_ENDS=0, read at every load, leaves
        // none: the same tables, every absent key on the ftab path (the A/B of profiles/r10_jump_absent.md)
        const char *ae = std::getenv("RBG_JUMP_ABSENT_ENDS");
        d.jump_complete = jump_complete_mask(JumpBuilt{true, words, keys}, JumpBuilt{l2.tab != nullptr, l2.words, l2.keys}, !(ae && ae[0] == '0'));
        if (std::getenv("RBG_VERBOSE"))
            std::fprintf(stderr, "rbg: device %d: jump table: level 1 %llu of %llu words inserted, level 2 %llu of %llu; an absent key ends the read at level%s\n",
                         ix->device, static_cast<unsigned long long>(keys), static_cast<unsigned long long>(words), static_cast<unsigned long long>(l2.tab ? l2.keys : 0),
                         static_cast<unsigned long long>(l2.words), d.jump_complete == 3 ? "s 1 and 2" : d.jump_complete == 1 ? " 1" : d.jump_complete == 2 ? " 2" : " none");
    } else if (std::getenv("RBG_VERBOSE")) {
        std::fprintf(stderr, "rbg: device %d: no jump table of %lld-mers (%llu occur): %s\n", ix->device, static_cast<long long>(jk),
                     static_cast<unsigned long long>(keys), why ? why : "skipped");
    }
    return RBG_OK;
}

// A load, step by step: each step is one of the functions above, the rules they apply are rbg_load_plan.hpp's.
int upload(rbg_index *ix) {
    LoadPlan p;
    int rc = check_device(ix, p);
    if (rc) return rc;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    if ((rc = compose_if_deferred(ix))) return rc;
    if ((rc = fix_budget(ix, p))) return rc;
    decide_layout(ix, p);
    if ((rc = second_look_at_layout(ix, p))) return rc;
    settle_layout(ix, p);
    if (p.runs_layout) trim_run_levels(ix, p);
    ix->kmer_steps_requested = std::max<uint64_t>(ix->kmer_steps_requested, static_cast<uint64_t>(levels_of(ix->H())));  // options_for() may have capped the depth already
    ix->hbm_free_at_load = p.free_b;
    ix->hbm_budget = p.budget;
    if (!p.runs_layout) trim_slot_levels(ix, p);
    say_what_is_kept(ix, p);
    if ((rc = upload_layout_tables(ix, p))) return rc;
    if ((rc = upload_small_arrays(ix, p))) return rc;
    if ((rc = build_ftab(ix))) return rc;
    return build_jump_table(ix);
}

FlattenOptions current_options() {
    FlattenOptions o;
    o.rank_bucket_shift = static_cast<int>(g_opt_rank_shift.load());
    o.deep_bucket_shift = static_cast<int>(g_opt_deep_shift.load());
    o.phi_bucket_shift = static_cast<int>(g_opt_phi_shift.load());
    o.force_pos_bytes = static_cast<int>(g_opt_pos_bytes.load());
    o.kmer_steps = static_cast<int>(g_opt_kmer_steps.load());
    return o;
}

// the k-mer tables of an index that goes to a device are composed there (RBG_HOST_COMPOSE=1: on the host, the reference
// statement -- A/B measurements and the test that compares the two)
bool host_compose_asked() {
    const char *e = std::getenv("RBG_HOST_COMPOSE");
    return e && e[0] == '1';
}
bool compose_deferred(int device) { return device != RBG_DEVICE_NONE && !host_compose_asked(); }

// The free HBM and the budget a load to `device` plans with, fixed while nothing of it is on the device (upload() measures again after the composition has
// taken its share, and a quarter of what is left then is not a quarter of the device): false where the device cannot be asked.
struct PlanMemory {
    size_t free_b = 0, whole_b = 0;   // whole_b: the device's memory (the assumed free memory where RBG_ASSUME_FREE_HBM_MB is set)
    int64_t opt_mb = 0;
    double budget = 0;
};
bool plan_memory(int device, PlanMemory &m) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return false;
    DeviceScope scope(device);
    if (scope.rc) return false;
    size_t total_b = 0;
    if (hipMemGetInfo(&m.free_b, &total_b) != hipSuccess) return false;
    const AssumedFree assumed = assumed_free_env();
    m.free_b = assumed_free_hbm(m.free_b, assumed.mb);
    m.whole_b = assumed.given ? m.free_b : total_b;
    m.opt_mb = g_opt_hbm_budget_mb.load();
    m.budget = static_cast<double>(load_budget(m.free_b, m.opt_mb, /*plan_budget=*/0));
    return true;
}

// Not even the single-symbol slot tables fit: the run-indexed layout, certainly (where the alphabet allows it) -- and RBG_LAYOUT_AUTO with no budget
// given may raise the budget for it (rbg_load_plan.hpp budget_raise): said on stderr, reported by rbg_info (hbm_budget) and rbg_layout_info
// (budget_raised); RBG_OPT_HBM_BUDGET_MB decides otherwise.
void plan_runs_of_a_large_index(int device, const RawRle &rle, const FlattenOptions &o, unsigned sigma, const PlanMemory &m, bool *auto_runs, rbg_index *ix) {
    if (sigma > static_cast<unsigned>(kLdsSyms)) return;
    *auto_runs = true;
    const double r = static_cast<double>(rle.heads.size());
    const BudgetRaise b = budget_raise(r, o.kmer_steps, m.free_b, m.whole_b, m.opt_mb, g_opt_rank_layout.load(), m.budget);
    if (!b.raise) return;
    std::fprintf(stderr, "rbg: device %d: r = %.3g runs: a quarter of the free HBM (%.1f GB) would leave fewer than %u symbols per step; RBG_LAYOUT_AUTO takes up to "
                         "three quarters (%.1f GB) for this index (RBG_OPT_HBM_BUDGET_MB sets the budget explicitly)\n", device, r, m.budget / 1e9, b.want, b.raised / 1e9);
    ix->plan_budget = static_cast<uint64_t>(b.raised);
    ix->budget_raised = true;
}

// The slot layout stages the tables of at most kMaxSlotKmerDepth symbols per gather (more are asked of the run-indexed layout only).  Levels that cannot
// fit the budget even in their smallest form (every table at the widest bucket) are not composed at all -- upload() would drop them anyway, and composing
// the deepest level is the most expensive part of flatten() (47 of 76 s at n = 5e10).  The bound is conservative: a level upload() could keep is never excluded.
void plan_slot_levels(int device, const RawRle &rle, FlattenOptions &o, unsigned sigma, double major, double budget, uint64_t *requested, bool *auto_runs) {
    const LoadConsts consts = load_consts();
    const int slot_steps = std::min(o.kmer_steps, kMaxSlotKmerDepth);
    const int keep = slot_levels_fitting(rle.n, major, slot_steps, kMaxWideShift, budget, consts);
    if (g_opt_rank_layout.load() == RBG_LAYOUT_AUTO && sigma <= static_cast<unsigned>(kLdsSyms) &&
        slot_levels_fitting(rle.n, major, slot_steps, kMaxNarrowShift, budget, consts) < slot_steps && runs_layout_fits(rle.heads.size(), budget)) {
        // RBG_LAYOUT_AUTO: slot tables only while those of every symbol per step fit the budget at their narrow buckets; rather than give up
        // symbols per step -- or widen the buckets -- the run-indexed layout (all of them, in space proportional to r; deeper steps than the
        // slot layout has: RBG_OPT_KMER_STEPS up to 8).  On the bench index 1.26e9 reads/s from 8.7 GB against 1.18e9 from the 59 GB of four
        // symbols per step (profiles/r04_bench.json space_speed); about 110 bytes per run at its leanest.
        if (std::getenv("RBG_VERBOSE"))
            std::fprintf(stderr, "rbg: device %d: the slot tables of %d symbols per step exceed the %.1f GB replica budget at narrow buckets: the run-indexed layout "
                                 "instead, %d symbols per step (RBG_OPT_RANK_LAYOUT = RBG_LAYOUT_PREFER_SLOTS keeps slot tables with fewer symbols)\n", device, slot_steps,
                         budget / 1e9, o.kmer_steps);
        *auto_runs = true;
        return;
    }
    if (keep >= o.kmer_steps) return;
    if (keep < slot_steps) {
        if (std::getenv("RBG_VERBOSE"))
            std::fprintf(stderr, "rbg: device %d: %.1f GB replica budget cannot hold k-mer levels beyond %d at n = %.3g: not composing them\n", device,
                         budget / 1e9, keep, static_cast<double>(rle.n));
        *requested = static_cast<uint64_t>(slot_steps);   // (what the slot layout could have taken of the depth asked for)
    }
    o.kmer_steps = keep;   // (the slot layout: at most kMaxSlotKmerDepth symbols per gather)
}

// The options of a load that is going to `device`.  *requested = the depth asked for when it was capped here (else 0: upload() reports what flatten()
// composed); *auto_runs: RBG_LAYOUT_AUTO chose the run-indexed layout already.
FlattenOptions options_for(int device, const RawRle &rle, uint64_t *requested, bool *auto_runs, rbg_index *ix) {
    FlattenOptions o = current_options();
    *requested = 0;
    *auto_runs = false;
    // A host-only handle (conversion, cache writing, tests) answers no query -- the library has no CPU search path -- so nothing reads k-mer
    // tables there: compose none (eight depths on the host cost 3 GB and a second per 3e6 runs, hundreds of GB at pangenome r: ADVICE r5).
    // (RBG_HOST_COMPOSE=1 keeps the host composition -- the serial reference statement of k_compose.hip -- reachable without a device: tests)
    if (device == RBG_DEVICE_NONE) {
        if (!host_compose_asked()) o.kmer_steps = 1;
        return o;
    }
    if (o.kmer_steps < 2) return o;
    PlanMemory m;
    if (!plan_memory(device, m)) return o;
    ix->plan_free = m.free_b;
    ix->plan_budget = static_cast<uint64_t>(m.budget);
    bool seen[256] = {};
    unsigned sigma = 0;
    for (uint8_t c : rle.heads)
        if (!seen[c]) { seen[c] = true; ++sigma; }
    const double major = static_cast<double>(std::min(4u, sigma > 1 ? sigma - 1 : 0u));  // at least this many k-mer symbols
    if (major < 2) return o;
    // the run-indexed layout keeps its k-mer depths as run lists (space proportional to r): nothing to cap when it is
    // asked for, or when not even the single-symbol slot tables (+ phi at its widest usual bucket) fit
    if (g_opt_rank_layout.load() == RBG_LAYOUT_RUNS) return o;
    const uint32_t pos_bytes = (o.force_pos_bytes == 8 || rle.n >= 0xFFFFFFF0ull) ? 8 : 4;
    if (layout_automatic() && slot_level1_estimate(rle.n, sigma, pos_bytes, load_consts()) > m.budget) {
        plan_runs_of_a_large_index(device, rle, o, sigma, m, auto_runs, ix);
        return o;
    }
    plan_slot_levels(device, rle, o, sigma, major, m.budget, requested, auto_runs);
    return o;
}

int upload_order_docs(rbg_index *ix);   // (below, beside rbg_set_docs)

int finish(rbg_index *ix, int device, rbg_index **out) {
    ix->device = device;
    if (device != RBG_DEVICE_NONE) {
        const auto t0 = std::chrono::steady_clock::now();
        int rc = upload(ix);
        if (!rc) rc = upload_order_docs(ix);   // (a document table loaded with the index: K3's chains in locus order)
        if (rc) { rbg_free(ix); return rc; }
        if (std::getenv("RBG_VERBOSE"))
            std::fprintf(stderr, "rbg: slot tables + upload %.2f s (%.2f GB)\n",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), ix->hbm_bytes / 1e9);
    }
    *out = ix;
    return RBG_OK;
}

bool markers_valid(const uint64_t *s, const uint64_t *e, uint64_t nruns, const uint64_t *off) {
    for (uint64_t j = 0; j < nruns; ++j) {
        if (e[j] < s[j] || off[j] > off[j + 1]) return false;
        if (j && s[j] <= e[j - 1]) return false;  // disjoint, ascending
    }
    return nruns == 0 || off[0] == 0;
}

bool file_readable(const std::string &fname) {
    FILE *f = std::fopen(fname.c_str(), "rb");
    if (!f) return false;
    std::fclose(f);
    return true;
}

// the reference's serialised files -> decoded bundle (load_rowbowt, rowbowt_io.hpp:176-189)
int bundle_from_index_files(const char *prefix, int flags, FlatBundle &b) {
    const std::string pre(prefix);
    int rc = parse_rbwt(pre + ".rbwt", b.rle);  // rowbowt_io.hpp:17,179-182
    if (rc) return rc;
    if (flags & RBG_LOAD_SA) {  // :18,184
        if ((rc = parse_tsa(pre + ".tsa", b.tsa))) return rc;
        b.has_tsa = true;
    }
    if (flags & RBG_LOAD_MA) {  // :19,185
        if ((rc = parse_mab(pre + ".mab", b.ma))) return rc;
        if (!markers_valid(b.ma.start.data(), b.ma.end.data(), b.ma.start.size(), b.ma.off.data())) return RBG_EFORMAT;
        b.has_ma = true;
    }
    if (flags & RBG_LOAD_DL) {  // :20,186
        if ((rc = parse_docs(pre + ".docs", b.dl))) return rc;
        b.has_dl = true;
    }
    return RBG_OK;
}

// rb_build's raw inputs (rb_build.cpp:83-93) -> decoded bundle
int bundle_from_raw_files(const char *bwt_fname, const char *ssa_fname, const char *esa_fname, FlatBundle &b) {
    RawRle &rle = b.rle;
    int rc = read_raw_bwt(bwt_fname, rle);
    if (rc) return rc;
    if (ssa_fname) {
        std::vector<uint64_t> ssa, esa;
        if ((rc = read_raw_samples(ssa_fname, ssa)) || (rc = read_raw_samples(esa_fname, esa))) return rc;
        if (ssa.size() != rle.R || esa.size() != rle.R) return RBG_EFORMAT;  // one sample pair per BWT run
        for (uint64_t i = 0; i < rle.R; ++i)
            if (ssa[i] > rle.n || esa[i] > rle.n) return RBG_EFORMAT;
        tsa_from_samples(rle.n, rle.R, ssa.data(), esa.data(), b.tsa);
        for (uint64_t j = 1; j < rle.R; ++j)
            if (b.tsa.pred_pos[j] == b.tsa.pred_pos[j - 1]) return RBG_EFORMAT;  // run-start samples must be distinct
        b.has_tsa = true;
    }
    return RBG_OK;
}

// RowBowt::build_ftab(k) + FTab::serialize (rowbowt.hpp:726-744, ftab.hpp:29-34): one text line
// "<kmer> <lo> <hi>" for every k-mer over ACGT with a non-empty range, in std::map (lexicographic)
// order, produced chunk by chunk; sink(text) returns false to stop early
template <typename Sink>
int ftab_stream(rbg_index *ix, uint64_t k, Sink sink) {
    const uint64_t total = uint64_t(1) << (2 * k);
    const uint64_t chunk = std::min<uint64_t>(total, uint64_t(1) << 21);
    std::vector<uint8_t> seqs(chunk * k);
    std::vector<uint64_t> off(chunk + 1), lo(chunk), hi(chunk);
    for (uint64_t i = 0; i <= chunk; ++i) off[i] = i * k;
    std::string text;
    for (uint64_t base = 0; base < total; base += chunk) {
        for (uint64_t i = 0; i < chunk; ++i) {
            const uint64_t L = base + i;  // lexicographic rank: first character most significant
            for (uint64_t j = 0; j < k; ++j) seqs[i * k + j] = static_cast<uint8_t>("ACGT"[(L >> (2 * (k - 1 - j))) & 3]);
        }
        const int rc = rbg_find_range(ix, seqs.data(), off.data(), chunk, lo.data(), hi.data());
        if (rc) return rc;
        text.clear();
        for (uint64_t i = 0; i < chunk; ++i) {
            if (lo[i] > hi[i]) continue;  // rowbowt.hpp:737
            text.append(reinterpret_cast<const char *>(&seqs[i * k]), k);
            text += ' ';
            text += std::to_string(lo[i]);
            text += ' ';
            text += std::to_string(hi[i]);
            text += '\n';
        }
        if (!sink(text)) break;
    }
    return RBG_OK;
}

int index_from_bundle(FlatBundle &b, int device, rbg_index **out) {
    rbg_index *ix = new (std::nothrow) rbg_index();
    if (!ix) return RBG_ENOMEM;
    FlattenOptions fo = options_for(device, b.rle, &ix->kmer_steps_requested, &ix->auto_runs, ix);
    fo.defer_kmer = compose_deferred(device);
    int rc = flatten(b.rle, b.has_tsa ? &b.tsa : nullptr, fo, ix->host);
    if (rc) { delete ix; return rc; }
    // (the flat index holds everything the bundle held: 33 bytes per run given back before the upload's own scratch is made)
    { RawRle().heads.swap(b.rle.heads); std::vector<uint64_t>().swap(b.rle.lens); RawTsa empty; std::swap(b.tsa, empty); }
    if (b.has_ma) { ix->H().ma = std::move(b.ma); ix->H().has_ma = true; }
    if (b.has_dl) { ix->H().dl = std::move(b.dl); ix->H().has_dl = true; }
    return finish(ix, device, out);
}

// No exception leaves the C ABI: a corrupt file that makes a reader allocate absurdly, or plain memory
// exhaustion on the host, comes back as an error code (the callers are C, cgo-style bindings, ctypes).
template <typename F>
int guarded(F &&f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        return RBG_ENOMEM;
    } catch (const std::length_error &) {
        return RBG_ENOMEM;
    } catch (...) {
        return RBG_EFORMAT;
    }
}

}  // namespace

namespace {
struct Reloc {
    std::vector<DevAlloc> from, to;
    const void *operator()(const void *p) const {
        if (!p) return nullptr;
        const char *c = static_cast<const char *>(p);
        for (size_t i = 0; i < from.size(); ++i) {
            const char *b = static_cast<const char *>(from[i].p);
            if (c >= b && c < b + from[i].bytes) return static_cast<const char *>(to[i].p) + (c - b);
        }
        return nullptr;  // not a pointer into the replica
    }
    template <typename T> void fix(T *&p) const { p = static_cast<T *>(const_cast<void *>((*this)(p))); }
};
}  // namespace

extern "C" {

int rbg_abi_version(void) { return RBG_ABI_VERSION; }

const char *rbg_strerror(int code) {
    switch (code) {
        case RBG_OK: return "ok";
        case RBG_EIO: return "file missing or unreadable";
        case RBG_EFORMAT: return "not the sdsl layout written by the reference";
        case RBG_ENODEV: return "no usable gfx950 device / HIP error (there is no CPU path)";
        case RBG_EARG: return "bad argument";
        case RBG_ENOMEM: return "out of memory";
        case RBG_ENOTLOADED: return "required structure (toehold SA / markers / docs) not loaded";
        default: return "unknown error";
    }
}

int rbg_set_default_option(int opt, int64_t value) {
    return guarded([&]() -> int {
    switch (opt) {
        case RBG_OPT_BLOCK_THREADS:
            if (value < 64 || value > 256 || value % 64) return RBG_EARG;  // kernels are built for <= 4 waves per workgroup
            g_opt_block_threads = value; return RBG_OK;
        case RBG_OPT_RANK_BUCKET_SHIFT:
            if (value < -1 || value > 12) return RBG_EARG;  // 8-bit slot offsets up to 8, the wide encoding up to 12
            g_opt_rank_shift = value; return RBG_OK;
        case RBG_OPT_DEEP_BUCKET_SHIFT:
            if (value < -1 || value > 12) return RBG_EARG;
            g_opt_deep_shift = value; return RBG_OK;
        case RBG_OPT_DENSE_OVERFLOW:
            if (value != 0 && value != 1) return RBG_EARG;
            g_opt_dense_overflow = value; return RBG_OK;
        case RBG_OPT_PHI_BUCKET_SHIFT:
            if (value < -1 || value > 8) return RBG_EARG;
            g_opt_phi_shift = value; return RBG_OK;
        case RBG_OPT_POS_BYTES:
            if (value != 0 && value != 4 && value != 8) return RBG_EARG;
            g_opt_pos_bytes = value; return RBG_OK;
        case RBG_OPT_FTAB_K:
            if (value < -1 || value > 16) return RBG_EARG;
            g_opt_ftab_k = value; return RBG_OK;
        case RBG_OPT_HBM_BUDGET_MB:
            if (value < 0) return RBG_EARG;
            g_opt_hbm_budget_mb = value; return RBG_OK;
        case RBG_OPT_KMER_STEPS:
            if (value < 1 || value > kMaxKmerDepth) return RBG_EARG;
            g_opt_kmer_steps = value; return RBG_OK;
        case RBG_OPT_PACKED_READS:
            if (value < 0 || value > 2) return RBG_EARG;
            g_opt_packed_reads = value; return RBG_OK;
        case RBG_OPT_RANK_LAYOUT:
            if (value != RBG_LAYOUT_AUTO && value != RBG_LAYOUT_SLOTS && value != RBG_LAYOUT_RUNS && value != RBG_LAYOUT_PREFER_SLOTS) return RBG_EARG;
            g_opt_rank_layout = value; return RBG_OK;
        case RBG_OPT_RUN_DEPTHS:
            if (value < 0 || value >= (1 << kMaxRunDepth)) return RBG_EARG;
            g_opt_run_depths = value; return RBG_OK;
        case RBG_OPT_RUN_PHI:
            if (value < 0 || value > 2) return RBG_EARG;
            g_opt_run_phi = value; return RBG_OK;
        case RBG_OPT_RUN_REC:
            if (value < 0 || value > 2) return RBG_EARG;
            g_opt_run_rec = value; return RBG_OK;
        case RBG_OPT_RUN_REC_DEPTHS:
            if (value < 0 || value >= (1 << kMaxRunDepth)) return RBG_EARG;
            g_opt_run_rec_depths = value; return RBG_OK;
        case RBG_OPT_JUMP_K:
            if (value < -1 || value > static_cast<int64_t>(kJumpMaxK) || (value > 0 && value < static_cast<int64_t>(kJumpMinK))) return RBG_EARG;
            g_opt_jump_k = value; return RBG_OK;
        case RBG_OPT_JUMP2_K:
            if (value < -1 || value > static_cast<int64_t>(kJump2MaxK) || (value > 0 && value < static_cast<int64_t>(kJump2MinK))) return RBG_EARG;
            g_opt_jump2_k = value; return RBG_OK;
        case RBG_OPT_EXTRACT_CHUNK:
            if (value < 1 || value > (int64_t(1) << 30)) return RBG_EARG;
            g_opt_extract_chunk = value; return RBG_OK;
        default: return RBG_EARG;
    }
    });
}

int rbg_get_default_option(int opt, int64_t *value) {
    return guarded([&]() -> int {
    if (!value) return RBG_EARG;
    switch (opt) {
        case RBG_OPT_BLOCK_THREADS: *value = g_opt_block_threads.load(); return RBG_OK;
        case RBG_OPT_RANK_BUCKET_SHIFT: *value = g_opt_rank_shift.load(); return RBG_OK;
        case RBG_OPT_DEEP_BUCKET_SHIFT: *value = g_opt_deep_shift.load(); return RBG_OK;
        case RBG_OPT_DENSE_OVERFLOW: *value = g_opt_dense_overflow.load(); return RBG_OK;
        case RBG_OPT_PHI_BUCKET_SHIFT: *value = g_opt_phi_shift.load(); return RBG_OK;
        case RBG_OPT_POS_BYTES: *value = g_opt_pos_bytes.load(); return RBG_OK;
        case RBG_OPT_FTAB_K: *value = g_opt_ftab_k.load(); return RBG_OK;
        case RBG_OPT_HBM_BUDGET_MB: *value = g_opt_hbm_budget_mb.load(); return RBG_OK;
        case RBG_OPT_KMER_STEPS: *value = g_opt_kmer_steps.load(); return RBG_OK;
        case RBG_OPT_PACKED_READS: *value = g_opt_packed_reads.load(); return RBG_OK;
        case RBG_OPT_RANK_LAYOUT: *value = g_opt_rank_layout.load(); return RBG_OK;
        case RBG_OPT_RUN_DEPTHS: *value = g_opt_run_depths.load(); return RBG_OK;
        case RBG_OPT_RUN_PHI: *value = g_opt_run_phi.load(); return RBG_OK;
        case RBG_OPT_RUN_REC: *value = g_opt_run_rec.load(); return RBG_OK;
        case RBG_OPT_RUN_REC_DEPTHS: *value = g_opt_run_rec_depths.load(); return RBG_OK;
        case RBG_OPT_JUMP_K: *value = g_opt_jump_k.load(); return RBG_OK;
        case RBG_OPT_JUMP2_K: *value = g_opt_jump2_k.load(); return RBG_OK;
        case RBG_OPT_EXTRACT_CHUNK: *value = g_opt_extract_chunk.load(); return RBG_OK;
        default: return RBG_EARG;
    }
    });
}

int rbg_load(const char *prefix, int flags, int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!prefix || !out) return RBG_EARG;
    *out = nullptr;
    FlatBundle b;
    int rc = bundle_from_index_files(prefix, flags, b);
    // no .rbwt but a native cache next to where it would be: use that (rb_build of this engine writes it);
    // a requested part the cache does not hold is still looked for in its own file (.docs is plain text
    // that rb_build copies, rowbowt_io.hpp:73-80)
    if (rc == RBG_EIO && !file_readable(std::string(prefix) + ".rbwt") && file_readable(std::string(prefix) + ".rbgpu")) {
        const std::string pre(prefix);
        FlatBundle c;
        if ((rc = read_flat(pre + ".rbgpu", c))) return rc;
        if ((flags & RBG_LOAD_SA) && !c.has_tsa) {
            if ((rc = parse_tsa(pre + ".tsa", c.tsa))) return rc;
            if (c.tsa.r != c.rle.R || c.tsa.n != c.rle.n) return RBG_EFORMAT;
            c.has_tsa = true;
        }
        if ((flags & RBG_LOAD_MA) && !c.has_ma) {
            if ((rc = parse_mab(pre + ".mab", c.ma))) return rc;
            if (!markers_valid(c.ma.start.data(), c.ma.end.data(), c.ma.start.size(), c.ma.off.data())) return RBG_EFORMAT;
            c.has_ma = true;
        }
        if ((flags & RBG_LOAD_DL) && !c.has_dl) {
            if ((rc = parse_docs(pre + ".docs", c.dl))) return rc;
            c.has_dl = true;
        }
        c.has_tsa = c.has_tsa && (flags & RBG_LOAD_SA);
        c.has_ma = c.has_ma && (flags & RBG_LOAD_MA);
        c.has_dl = c.has_dl && (flags & RBG_LOAD_DL);
        return index_from_bundle(c, device, out);
    }
    if (rc) return rc;
    return index_from_bundle(b, device, out);
    });
}

int rbg_load_cache(const char *path, int flags, int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!path || !out) return RBG_EARG;
    *out = nullptr;
    FlatBundle b;
    int rc = read_flat(path, b);
    if (rc) return rc;
    // a part the caller asks for must be in the file, like a missing .tsa/.mab/.docs (rowbowt_io.hpp:166-169)
    if (((flags & RBG_LOAD_SA) && !b.has_tsa) || ((flags & RBG_LOAD_MA) && !b.has_ma) || ((flags & RBG_LOAD_DL) && !b.has_dl))
        return RBG_EIO;
    b.has_tsa = b.has_tsa && (flags & RBG_LOAD_SA);
    b.has_ma = b.has_ma && (flags & RBG_LOAD_MA);
    b.has_dl = b.has_dl && (flags & RBG_LOAD_DL);
    return index_from_bundle(b, device, out);
    });
}

int rbg_convert_index(const char *prefix, int flags, const char *out_path) {
    return guarded([&]() -> int {
    if (!prefix || !out_path) return RBG_EARG;
    FlatBundle b;
    int rc = bundle_from_index_files(prefix, flags, b);
    if (rc) return rc;
    return write_flat(out_path, b);
    });
}

int rbg_convert_raw(const char *bwt_fname, const char *ssa_fname, const char *esa_fname, const char *mab_fname,
                    const char *docs_fname, const char *out_path) {
    return guarded([&]() -> int {
    if (!bwt_fname || !out_path || (!!ssa_fname != !!esa_fname)) return RBG_EARG;
    FlatBundle b;
    int rc = bundle_from_raw_files(bwt_fname, ssa_fname, esa_fname, b);
    if (rc) return rc;
    if (mab_fname) {
        if ((rc = parse_mab(mab_fname, b.ma))) return rc;
        if (!markers_valid(b.ma.start.data(), b.ma.end.data(), b.ma.start.size(), b.ma.off.data())) return RBG_EFORMAT;
        b.has_ma = true;
    }
    if (docs_fname) {
        if ((rc = parse_docs(docs_fname, b.dl))) return rc;
        b.has_dl = true;
    }
    return write_flat(out_path, b);
    });
}

// a run-length BWT (+ both samples of every run) in memory -> the native cache file (what rbg_convert_raw writes for
// the same index from its .bwt/.ssa/.esa files): for builders that never materialise the BWT as text -- n = 5e10 would be
// a 50 GB .bwt -- and for handing one index to several processes of a node (bench.py: rank 0 writes, every rank loads)
static int runs_to_bundle(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y, const uint64_t *esa_y, FlatBundle &b);

int rbg_convert_runs(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y, const uint64_t *esa_y, const char *out_path) {
    return rbg_convert_runs_markers(heads, lens, R, ssa_y, esa_y, nullptr, nullptr, 0, nullptr, nullptr, nullptr, out_path);
}

int rbg_convert_runs_markers(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y, const uint64_t *esa_y,
                             const uint64_t *mk_start, const uint64_t *mk_end, uint64_t mk_nruns, const uint64_t *mk_off, const uint64_t *mk_vals,
                             const char *docs_text, const char *out_path) {
    return guarded([&]() -> int {
    if (!heads || !lens || !out_path || R == 0 || (!!ssa_y != !!esa_y)) return RBG_EARG;
    if (mk_nruns && (!mk_start || !mk_end || !mk_off || !mk_vals)) return RBG_EARG;
    FlatBundle b;
    int rc = runs_to_bundle(heads, lens, R, ssa_y, esa_y, b);
    if (rc) return rc;
    if (mk_nruns) {
        if (!markers_valid(mk_start, mk_end, mk_nruns, mk_off)) return RBG_EARG;
        if (mk_end[mk_nruns - 1] >= b.rle.n) return RBG_EARG;
        b.ma.start.assign(mk_start, mk_start + mk_nruns);
        b.ma.end.assign(mk_end, mk_end + mk_nruns);
        b.ma.off.assign(mk_off, mk_off + mk_nruns + 1);
        b.ma.vals.assign(mk_vals, mk_vals + mk_off[mk_nruns]);
        b.has_ma = true;
    }
    if (docs_text) {   // the text of a .docs file (doclist.hpp:57-73: whitespace-separated name / start pairs)
        std::istringstream ss{std::string(docs_text)};
        std::string name;
        uint64_t pos = 0;
        while (ss >> name >> pos) { b.dl.names.push_back(name); b.dl.starts.push_back(pos); }
        if (b.dl.names.empty()) return RBG_EARG;
        b.dl.sorted = b.dl.starts;
        std::sort(b.dl.sorted.begin(), b.dl.sorted.end());
        b.has_dl = true;
    }
    return write_flat(out_path, b);
    });
}

int rbg_build_from_runs(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y,
                        const uint64_t *esa_y, int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!heads || !lens || !out || R == 0 || (!!ssa_y != !!esa_y)) return RBG_EARG;
    *out = nullptr;
    FlatBundle b;
    const int rc0 = runs_to_bundle(heads, lens, R, ssa_y, esa_y, b);
    if (rc0) return rc0;
    return index_from_bundle(b, device, out);
    });
}

static int runs_to_bundle(const uint8_t *heads, const uint64_t *lens, uint64_t R, const uint64_t *ssa_y, const uint64_t *esa_y, FlatBundle &bundle) {
    {
    RawRle &rle = bundle.rle;
    RawTsa &tsa = bundle.tsa;
    bundle.has_tsa = ssa_y != nullptr;
    rle.R = R;
    rle.B = 2;
    rle.heads.resize(R);
    rle.lens.resize(R);
    // (every loop over the runs is split over the worker threads: 3e8 runs at pangenome scale)
    const unsigned T = load_threads();
    std::vector<uint64_t> part(T + 1, 0);
    std::vector<int> bad(T + 1, 0);
    parallel_for(R, [&](uint64_t b, uint64_t e, unsigned t) {
        uint64_t sum = 0;
        for (uint64_t i = b; i < e; ++i) {
            if (lens[i] == 0 || (i && heads[i] == heads[i - 1])) bad[t] = 1;  // runs are non-empty and maximal
            sum += lens[i];
            rle.heads[i] = heads[i];
            rle.lens[i] = lens[i];
        }
        part[t] = sum;
    });
    uint64_t n = 0;
    for (unsigned t = 0; t <= T; ++t) { if (bad[t]) return RBG_EARG; n += part[t]; }
    rle.n = n;
    if (ssa_y) {
        parallel_for(R, [&](uint64_t b, uint64_t e, unsigned t) {
            for (uint64_t i = b; i < e; ++i)
                if (ssa_y[i] > n || esa_y[i] > n) bad[t] = 1;  // SA values of an n-symbol text
        });
        for (unsigned t = 0; t <= T; ++t) if (bad[t]) return RBG_EARG;
        tsa_from_samples(n, R, ssa_y, esa_y, tsa);
        parallel_for(R, [&](uint64_t b, uint64_t e, unsigned t) {
            for (uint64_t j = std::max<uint64_t>(b, 1); j < e; ++j)
                if (tsa.pred_pos[j] == tsa.pred_pos[j - 1]) bad[t] = 1;  // run-start samples must be distinct
        });
        for (unsigned t = 0; t <= T; ++t) if (bad[t]) return RBG_EARG;
    }
    return RBG_OK;
    }
}

int rbg_build_from_files(const char *bwt_fname, const char *ssa_fname, const char *esa_fname, int device, rbg_index **out) {
    return guarded([&]() -> int {
    if (!bwt_fname || !out || (!!ssa_fname != !!esa_fname)) return RBG_EARG;
    *out = nullptr;
    FlatBundle b;
    int rc = bundle_from_raw_files(bwt_fname, ssa_fname, esa_fname, b);
    if (rc) return rc;
    return index_from_bundle(b, device, out);
    });
}

int rbg_write_ftab(rbg_index *ix, uint64_t k, const char *path) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!path || k == 0 || k > 16) return RBG_EARG;
    FILE *fp = std::fopen(path, "wb");
    if (!fp) return RBG_EIO;
    bool io_ok = true;
    int rc = ftab_stream(ix, k, [&](const std::string &t) {
        if (!t.empty() && std::fwrite(t.data(), 1, t.size(), fp) != t.size()) io_ok = false;
        return io_ok;
    });
    if (std::fclose(fp) != 0) io_ok = false;
    if (!rc && !io_ok) rc = RBG_EIO;
    return rc;
    });
}

// FTab::load (ftab.hpp:15-27) keeps k = length of the last line's k-mer.  The file is accepted only if
// it is, byte for byte, the table build_ftab(k) gives for this index: then search_ftab(q) is
// "find_range(q) when q is over ACGT and occurs", which is how the ftab variants are computed here.
int rbg_check_ftab(rbg_index *ix, const char *path, uint64_t *k_out) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!path || !k_out) return RBG_EARG;
    *k_out = 0;
    FILE *fp = std::fopen(path, "rb");
    if (!fp) return RBG_EIO;
    char first[64];
    uint64_t k = 0;
    if (std::fgets(first, sizeof first, fp)) while (k < sizeof first && first[k] && first[k] != ' ' && first[k] != '\n') ++k;
    if (k == 0 || k > 16) { std::fclose(fp); return RBG_EFORMAT; }
    std::rewind(fp);
    bool same = true;
    std::vector<char> buf;
    int rc = ftab_stream(ix, k, [&](const std::string &t) {
        buf.resize(t.size());
        if (!t.empty() && (std::fread(buf.data(), 1, t.size(), fp) != t.size() || std::memcmp(buf.data(), t.data(), t.size()) != 0)) same = false;
        return same;
    });
    if (!rc && same && std::fgetc(fp) != EOF) same = false;  // nothing may follow
    std::fclose(fp);
    if (rc) return rc;
    if (!same) return RBG_EFORMAT;
    *k_out = k;
    return RBG_OK;
    });
}

int rbg_set_markers(rbg_index *ix, const uint64_t *run_start, const uint64_t *run_end, uint64_t nruns,
                    const uint64_t *mk_off, const uint64_t *mk_vals) {
    return guarded([&]() -> int {
    if (!ix || !run_start || !run_end || !mk_off || (!mk_vals && mk_off[nruns])) return RBG_EARG;
    if (!markers_valid(run_start, run_end, nruns, mk_off)) return RBG_EARG;
    if (ix->primary) return RBG_EARG;    // attach to the primary, before rbg_replicate
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->H().has_ma) return RBG_EARG;  // immutable once attached
    RawMarkers &m = ix->H().ma;
    m.start.assign(run_start, run_start + nruns);
    m.end.assign(run_end, run_end + nruns);
    m.off.assign(mk_off, mk_off + nruns + 1);
    m.vals.assign(mk_vals, mk_vals + mk_off[nruns]);
    ix->H().has_ma = true;
    if (ix->device != RBG_DEVICE_NONE) {
        DeviceScope scope(ix->device);
        if (scope.rc) return scope.rc;
        return upload_markers(ix);
    }
    return RBG_OK;
    });
}

}  // extern "C"
namespace {
// the document starts on the device for K3's locus order (rbg_dev.h order_docs).  RBG_LOCATE_ORDER=abs keeps the order by absolute position.
int upload_order_docs(rbg_index *ix) {
    DevIndex &d = ix->dev;
    if (d.order_docs && ix->device != RBG_DEVICE_NONE && !ix->primary) {
        // a table attached before: its array goes back (it would be copied to every replica and counted in hbm_bytes), whether or not the new table gets
        // one (the order may have become ineligible) -- rbg_set_docs must not overlap queries on the handle (include/rbg.h)
        DeviceScope scope(ix->device);
        if (scope.rc) return scope.rc;
        HIP_TRY(hipDeviceSynchronize());
        free_tracked(ix, const_cast<uint64_t *>(d.order_docs));
    }
    d.order_docs = nullptr;
    d.order_ndocs = d.order_dbits = d.order_lowbits = d.order_obits = 0;
    if (ix->device == RBG_DEVICE_NONE || ix->primary) return RBG_OK;
    // RBG_LOCATE_ORDER = abs: never; locus: whenever there are two documents or more; unset: from 128 documents on -- measured (profiles/
    // r06_locus_order_ab.txt): K3 53.7 -> 50.4 ms per 10 M x 150 bp reads at r = 1.07e9 / 520 haplotypes, equal at 200 haplotypes, and on the bench
    // index (50 haplotypes) the key pass and the wider sort cost more (0.17 ms) than K3 gains (0.02 ms).
    const char *e = std::getenv("RBG_LOCATE_ORDER");
    if (e && std::strcmp(e, "abs") == 0) return RBG_OK;
    const bool forced = e && std::strcmp(e, "locus") == 0;
    const RawDocs &dl = ix->H().dl;
    const uint64_t nd = dl.sorted.size();
    if (!ix->H().has_dl || nd < (forced ? 2u : 128u) || nd > (uint64_t(1) << 20) || dl.sorted[0] != 0) return RBG_OK;   // (one document: the absolute order already is the locus order)
    uint64_t longest = 0;
    for (uint64_t j = 0; j < nd; ++j) longest = std::max(longest, (j + 1 < nd ? dl.sorted[j + 1] : ix->H().n) - dl.sorted[j]);
    uint32_t obits = 1, dbits = 1;
    while (obits < 64 && (longest >> obits)) ++obits;
    while ((nd >> dbits)) ++dbits;
    if (obits + dbits > 60) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    // (an allocation of its own, never a piece of the arena: free_tracked must be able to give it back when another table replaces this one)
    void *p = nullptr;
    const size_t alloc = arena_round(nd * 8);
    HIP_TRY(hipMalloc(&p, alloc));
    ix->allocs.push_back({p, alloc});
    ix->hbm_bytes += alloc;
    if (const int rc = h2d_big(p, dl.sorted.data(), nd * 8)) { free_tracked(ix, p); return rc; }
    d.order_docs = static_cast<const uint64_t *>(p);
    d.order_ndocs = static_cast<uint32_t>(nd);
    d.order_dbits = dbits;
    d.order_obits = obits;
    // positions inside one line of phi slots need no sorting (as in the absolute order: launch_locate_order's begin_bit)
    d.order_lowbits = std::min<uint32_t>(d.phi_shift + 2u, obits > 8 ? obits - 8 : 0u);
    return RBG_OK;
}
}  // namespace
extern "C" {

int rbg_set_docs(rbg_index *ix, const char *names_joined, const uint64_t *starts, uint64_t ndocs) {
    return guarded([&]() -> int {
    if (!ix || !names_joined || !starts || ix->primary) return RBG_EARG;
    std::lock_guard<std::mutex> g(ix->mu);
    RawDocs &d = ix->H().dl;
    d = RawDocs();
    const char *p = names_joined;
    for (uint64_t i = 0; i < ndocs; ++i) {
        d.names.emplace_back(p);
        p += d.names.back().size() + 1;
        d.starts.push_back(starts[i]);
    }
    d.sorted = d.starts;
    std::sort(d.sorted.begin(), d.sorted.end());
    ix->H().has_dl = true;
    {   // rbg_align_text keeps a device copy of the table: made again at its next call (the old arrays stay until rbg_free)
        std::lock_guard<std::mutex> g2(ix->text_mu);
        ix->text_docs = rbg_index::TextDocs();
    }
    drop_doc_dev(ix);   // rbg_docs_prepare's copy is of the table before: prepare again (a replica's copy goes stale by the count)
    ++ix->docs_gen;
    return upload_order_docs(ix);   // (K3's chain order by locus: attach the documents BEFORE replicating, like the markers)
    });
}

void rbg_free(rbg_index *ix) {
    if (!ix) return;
    if (ix->device != RBG_DEVICE_NONE) {
        DeviceScope scope(ix->device);
        ix->ws_free.clear();  // pinned + device staging of the host-pointer calls
        for (auto &t : ix->text_out) {
            if (t.pending) (void)hipEventSynchronize(t.done);
            if (t.d_text) DevPool::get().release(t.d_text, t.d_cls, t.d_dev);
            if (t.done) (void)hipEventDestroy(t.done);
            (void)hipHostFree(t.p);
        }
        if (ix->text_copy_stream) (void)hipStreamDestroy(ix->text_copy_stream);
        for (auto &t : ix->text_in) (void)hipHostFree(t.p);
        for (const DevAlloc &a : ix->allocs) (void)hipFree(a.p);
        DevPool::get().trim(ix->device);  // cached scratch blocks of the host-pointer calls
    }
    delete ix;
}

void rbg_free_buffer(void *p) {
    if (!p) return;
    ResultPool &P = ResultPool::get();
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.live.find(p);
        if (it != P.live.end()) {
            const size_t size = it->second;
            P.live.erase(it);
            if (P.on && P.cached + size <= ResultPool::kMax) {
                P.idle.emplace(size, p);
                P.cached += size;
                return;
            }
        }
    }
    std::free(p);
}

// rbg_info for a caller compiled against ANOTHER layout of rbg_info_t (the struct grew with ABI 3 and rbg_info cannot know what its caller
// allocated): fills min(out_bytes, sizeof(rbg_info_t)) bytes -- fields are only ever added at the end from ABI 3 on.
int rbg_info_sized(const rbg_index *ix, rbg_info_t *out, uint64_t out_bytes) {
    if (!ix || !out || out_bytes < 8) return RBG_EARG;
    rbg_info_t v;
    const int rc = rbg_info(ix, &v);
    if (rc) return rc;
    std::memcpy(out, &v, static_cast<size_t>(std::min<uint64_t>(out_bytes, sizeof(v))));
    return RBG_OK;
}

// min(out_bytes, sizeof(rbg_jump_info_t)) bytes: the struct grew by level 2 and by `complete`, each time at its end (as rbg_info_sized)
int rbg_jump_info_sized(const rbg_index *ix, rbg_jump_info_t *out, uint64_t out_bytes) {
    return guarded([&]() -> int {
    if (!ix || !out || out_bytes < 8) return RBG_EARG;
    const rbg_index *s = ix->primary ? ix->primary : ix;   // (a replica holds a copy of its primary's tables)
    rbg_jump_info_t v;
    std::memset(&v, 0, sizeof(v));
    if (ix->dev.jump) {
        v.k = ix->dev.jump_k;
        v.keys = s->jump_keys;
        v.bytes = s->jump_bytes;
        v.buckets = ix->dev.jump_buckets;
        v.build_ms = s->jump_build_ms;
    }
    if (ix->dev.jump2_k) {
        v.k2 = ix->dev.jump2_k;
        v.keys2 = s->jump2_keys;
        v.bytes2 = s->jump2_bytes;
        v.buckets2 = ix->dev.jump2_buckets;
        v.build2_ms = s->jump2_build_ms;
    }
    if (ix->dev.jump) v.complete = ix->dev.jump_complete;
    std::memcpy(out, &v, static_cast<size_t>(std::min<uint64_t>(out_bytes, sizeof(v))));
    return RBG_OK;
    });
}

// the caller of before level 2: the five fields the struct had then, and not a byte more
int rbg_jump_info(const rbg_index *ix, rbg_jump_info_t *out) {
    return rbg_jump_info_sized(ix, out, offsetof(rbg_jump_info_t, k2));
}

int rbg_info(const rbg_index *ix, rbg_info_t *out) {
    return guarded([&]() -> int {
    if (!ix || !out) return RBG_EARG;
    std::memset(out, 0, sizeof(*out));
    out->n = ix->H().n;
    out->r = ix->H().r;
    out->sigma = ix->H().sigma;
    out->pos_bytes = ix->H().pos_bytes;
    out->device = ix->device;
    out->has_tsa = ix->H().has_tsa;
    out->has_markers = ix->H().has_ma;
    out->has_docs = ix->H().has_dl;
    out->hbm_bytes = ix->hbm_bytes;
    out->marker_runs = ix->H().ma.start.size();
    out->marker_vals = ix->H().ma.vals.size();
    out->rank_bucket_shift = ix->H().sym.empty() ? 0 : ix->H().sym.back().shift;
    out->phi_bucket_shift = ix->H().phi_shift;
    out->rank_slots = ix->rank_slots;
    out->rank_slots_overflow = ix->rank_slots_overflow;
    out->phi_slots = ix->phi_slots;
    out->phi_slots_overflow = ix->phi_slots_overflow;
    out->kmer_steps = ix->H().kmer_levels();
    if (ix->device != RBG_DEVICE_NONE && ix->dev.layout == RBG_LAYOUT_RUNS) out->kmer_steps = ix->dev.run_ksteps;   // depths of the run-indexed search
    out->kmer_symbols = ix->H().kmer(2).empty() ? 0 : ix->H().nmajor;
    out->slot_bytes = ix->device != RBG_DEVICE_NONE && ix->dev.layout == RBG_LAYOUT_SLOTS ? 16 : 0;
    out->ftab_k = ix->dev.ftab_k;
    out->kmer_steps_requested = ix->kmer_steps_requested ? ix->kmer_steps_requested : out->kmer_steps;
    out->hbm_free_at_load = ix->hbm_free_at_load;
    out->hbm_budget = ix->hbm_budget;
    out->rank_layout = ix->runs_layout ? RBG_LAYOUT_RUNS : RBG_LAYOUT_SLOTS;
    out->replicas = ix->device == RBG_DEVICE_NONE ? 0 : 1;
    out->depth_runs[0] = ix->H().r;
    const bool runs_dev = ix->device != RBG_DEVICE_NONE && ix->dev.layout == RBG_LAYOUT_RUNS;
    for (uint32_t d = 2; d <= static_cast<uint32_t>(kMaxKmerDepth); ++d) {
        if (runs_dev && !(ix->dev.run_depth_mask >> (d - 1) & 1u)) continue;   // depths left without run lists (RBG_OPT_RUN_DEPTHS) report none
        for (const SymTable &t : ix->H().kmer(d)) out->depth_runs[d - 1] += t.nruns;
    }
    out->pair_runs = out->depth_runs[1]; out->triple_runs = out->depth_runs[2]; out->quad_runs = out->depth_runs[3]; out->quint_runs = out->depth_runs[4];
    return RBG_OK;
    });
}

int rbg_layout_info(const rbg_index *ix, rbg_layout_info_t *out, uint64_t out_bytes) {
    return guarded([&]() -> int {
    if (!ix || !out || out_bytes < 8) return RBG_EARG;
    // (ABI 3 changed this struct in the middle -- five-entry arrays became eight -- so a size that is neither this layout's nor a prefix of it at
    //  an 8-byte boundary beyond the ABI-3 head is a caller compiled against ABI 2: refused rather than filled with shifted fields)
    if (out_bytes < offsetof(rbg_layout_info_t, budget_raised) && out_bytes != offsetof(rbg_layout_info_t, rec_bytes) && out_bytes != offsetof(rbg_layout_info_t, entries))
        return RBG_EARG;
    rbg_layout_info_t v;
    std::memset(&v, 0, sizeof(v));
    if (ix->device != RBG_DEVICE_NONE && ix->dev.layout == RBG_LAYOUT_RUNS) {
        const rbg_index::RunsReport &r = ix->runs_report;
        v.run_fmt = r.fmt;
        v.depths_composed = r.depths_composed;
        v.depth_mask_asked = r.depth_mask_asked;
        v.depth_mask_kept = r.depth_mask_kept;
        v.depths_dropped_budget = r.depths_dropped_budget;
        v.rank_directories = r.rank_dirs;
        v.phi_directory = r.phi_dir;
        v.fill_shift = r.fmt == 2 && ix->H().pos_bytes == 8 ? ix->dev.run_fill_shift : 0;
        for (int d = 0; d < kMaxRunDepth; ++d) { v.entries[d] = r.entries[d]; v.fillers[d] = r.fillers[d]; v.dir_bytes[d] = r.dir_bytes[d]; }
        v.phi_entries = r.phi_entries; v.phi_fillers = r.phi_fillers; v.phi_dir_bytes = r.phi_dir_bytes; v.phi_dir_shift = r.phi_dir_shift;
        v.phi_slots = r.phi_slots; v.phi_slot_bytes = r.phi_slot_bytes;
        for (int d = 0; d < kMaxRunDepth; ++d) { v.rec_bytes[d] = r.rec_bytes[d]; v.rec_overflow[d] = r.rec_overflow[d]; }
        v.budget_raised = ix->budget_raised ? 1 : 0;
    }
    std::memcpy(out, &v, static_cast<size_t>(std::min<uint64_t>(out_bytes, sizeof(v))));
    return RBG_OK;
    });
}

int rbg_get_f(const rbg_index *ix, uint64_t f_out[256]) {
    return guarded([&]() -> int {
    if (!ix || !f_out) return RBG_EARG;
    std::memcpy(f_out, ix->H().f, 256 * sizeof(uint64_t));
    return RBG_OK;
    });
}

int rbg_last_run_sample(const rbg_index *ix, uint64_t *out) {
    return guarded([&]() -> int {
    if (!ix || !out) return RBG_EARG;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    *out = ix->H().last_run_sample;
    return RBG_OK;
    });
}

int rbg_host_array(const rbg_index *ix, int which, uint64_t *dst, uint64_t cap, uint64_t *count) {
    return guarded([&]() -> int {
    if (!ix || !count) return RBG_EARG;
    const HostIndex &h = ix->H();
    const std::vector<uint64_t> *v = nullptr;
    std::vector<uint64_t> tmp;
    switch (which) {
        case RBG_ARR_RUN_HEADS: tmp.assign(h.run_heads.begin(), h.run_heads.end()); v = &tmp; break;
        case RBG_ARR_RUN_START: v = &h.run_start; break;
        case RBG_ARR_SAMPLES_LAST: v = &h.samples_last; break;
        case RBG_ARR_PRED_POS: v = &h.pred_pos; break;
        case RBG_ARR_PHI_BASE: v = &h.phi_base; break;
        case RBG_ARR_MARKER_START: v = &h.ma.start; break;
        case RBG_ARR_MARKER_END: v = &h.ma.end; break;
        case RBG_ARR_MARKER_OFF: v = &h.ma.off; break;
        case RBG_ARR_MARKER_VALS: v = &h.ma.vals; break;
        default: return RBG_EARG;
    }
    *count = v->size();
    if (dst) std::memcpy(dst, v->data(), std::min<uint64_t>(cap, v->size()) * 8);
    return RBG_OK;
    });
}

int rbg_resolve_offset(const rbg_index *ix, uint64_t i, const char **name, uint64_t *offset) {
    return guarded([&]() -> int {
    if (!ix || !name || !offset) return RBG_EARG;
    if (!ix->H().has_dl || ix->H().dl.names.empty()) return RBG_ENOTLOADED;
    const RawDocs &d = ix->H().dl;
    // DocList::doc_bounds_rank, doclist.hpp:77-79: rank(min(i+1, size)) over a bit-vector whose
    // size is the LAST start read + 1 (doclist.hpp:66)
    const uint64_t size = d.starts.back() + 1;
    const uint64_t q = i + 1 > size ? size : i + 1;
    const uint64_t rank = std::lower_bound(d.sorted.begin(), d.sorted.end(), q) - d.sorted.begin();
    if (rank == 0) return RBG_EARG;  // reference indexes doc_names_[-1] here
    *offset = i - d.sorted[rank - 1];           // doclist.hpp:48
    *name = d.names[rank - 1].c_str();          // doclist.hpp:49
    return RBG_OK;
    });
}

// The table rbg_resolve_offset answers from, for callers that resolve millions of positions (rb_align -s prints some
// forty per read): a call per position through the ABI was a third of that tool's formatting time.
int rbg_doc_table(rbg_index *ix, uint64_t *ndocs, const uint64_t **sorted_starts, const char *const **names, uint64_t *size) {
    return guarded([&]() -> int {
    if (!ix || !ndocs || !sorted_starts || !names || !size) return RBG_EARG;
    rbg_index *root = ix->primary ? ix->primary : ix;
    if (!root->H().has_dl || root->H().dl.names.empty()) return RBG_ENOTLOADED;
    const RawDocs &d = root->H().dl;
    {
        std::lock_guard<std::mutex> g(root->mu);
        if (root->doc_name_ptrs.size() != d.names.size()) {
            root->doc_name_ptrs.clear();
            for (const std::string &n : d.names) root->doc_name_ptrs.push_back(n.c_str());
        }
    }
    *ndocs = d.names.size();
    *sorted_starts = d.sorted.data();
    *names = root->doc_name_ptrs.data();
    *size = d.starts.back() + 1;
    return RBG_OK;
    });
}

}  // extern "C"
