// capi/docs.ipp -- the document table on the handle's device (rbg_docs_prepare; rbg_docdir.hpp: the rule and its directory), the device pair over K3's
// output (k_docs.hip: rbg_resolve_offsets_dev*, rbg_doc_hits_dev*), the walk that reduces as it goes (rbg_locate_docs.hpp: rbg_locate_doc_hits_dev) and the
// host-pointer composites rbg_doc_hits / rbg_doc_hits_locs.  Part of rbg_capi.hip.
namespace {
const rbg_index *doc_root(const rbg_index *ix) { return ix->primary ? ix->primary : ix; }
bool has_docs(const rbg_index *ix) {
    const RawDocs &d = ix->H().dl;
    return ix->H().has_dl && !d.names.empty() && d.starts.size() == d.names.size();
}
// the copy on this handle's device is of the table the root holds now
bool doc_dev_current(const rbg_index *ix) { return ix->doc_dev.sorted && ix->doc_dev.gen == doc_root(ix)->docs_gen; }

int docs_prepare(rbg_index *ix) {
    if (!queryable(ix)) return RBG_ENODEV;
    std::lock_guard<std::mutex> g(ix->mu);
    if (!has_docs(ix)) return RBG_ENOTLOADED;
    if (doc_dev_current(ix)) return RBG_OK;
    const RawDocs &d = ix->H().dl;
    DocDir D;
    if (!doc_dir_build(d.starts.data(), d.starts.size(), D)) return RBG_EARG;   // more than kDocMaxDocs documents
    drop_doc_dev(ix);   // (a copy of an earlier table)
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    // (allocations of their own, never pieces of the arena: free_tracked gives them back when another table replaces this one)
    void *p[2] = {nullptr, nullptr};
    const size_t bytes[2] = {D.sorted.size() * 8, D.dir.size() * 4};
    const void *src[2] = {D.sorted.data(), D.dir.data()};
    for (int k = 0; k < 2; ++k) {
        const size_t alloc = arena_round(bytes[k]);
        hipError_t e = hipMalloc(&p[k], alloc);
        if (e == hipSuccess) {
            ix->allocs.push_back({p[k], alloc});
            ix->hbm_bytes += alloc;
            e = hipMemcpy(p[k], src[k], bytes[k], hipMemcpyHostToDevice);
        } else {
            p[k] = nullptr;
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            free_tracked(ix, p[0]);
            if (k) free_tracked(ix, p[1]);
            return e == hipErrorOutOfMemory ? RBG_ENOMEM : RBG_ENODEV;
        }
    }
    rbg_index::DocDev &v = ix->doc_dev;
    v.sorted = static_cast<const uint64_t *>(p[0]);
    v.dir = static_cast<const uint32_t *>(p[1]);
    v.size = D.size;
    v.ndocs = static_cast<uint32_t>(D.sorted.size());
    v.shift = D.shift;
    v.ndir = static_cast<uint32_t>(D.dir.size());
    v.gen = doc_root(ix)->docs_gen;
    return RBG_OK;
}

int resolve_offsets_dev(rbg_index *ix, const void *d_locs, bool locs32, uint64_t M, uint32_t *d_doc, uint64_t *d_offset, void *stream) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!doc_dev_current(ix)) return RBG_ENOTLOADED;
    if (M && (!d_locs || !d_doc)) return RBG_EARG;
    const rbg_index::DocDev &v = ix->doc_dev;
    return launch_resolve_offsets(v.sorted, v.dir, v.size, v.ndocs, v.shift, v.ndir, d_locs, locs32, M, d_doc, d_offset, stream) ? RBG_ENODEV : RBG_OK;
}

int doc_hits_dev(rbg_index *ix, const void *d_locs, bool locs32, const uint64_t *d_loc_off, uint64_t N, uint64_t *d_sets, uint32_t *d_ndocs, uint32_t *d_nodoc,
                 uint64_t *d_doc_reads, void *stream) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!doc_dev_current(ix)) return RBG_ENOTLOADED;
    if (N && (!d_locs || !d_loc_off)) return RBG_EARG;
    if (!d_sets && !d_ndocs && !d_nodoc && !d_doc_reads) return RBG_OK;
    const rbg_index::DocDev &v = ix->doc_dev;
    return launch_doc_hits(v.sorted, v.dir, v.size, v.ndocs, v.shift, v.ndir, d_locs, locs32, d_loc_off, N, d_sets, d_ndocs, d_nodoc, d_doc_reads,
                           docs_group(), stream) ? RBG_ENODEV : RBG_OK;
}

DocTable doc_table_of(const rbg_index::DocDev &v) {
    DocTable t;
    t.sorted = v.sorted; t.dir = v.dir; t.size = v.size; t.ndocs = v.ndocs; t.shift = v.shift; t.ndir = v.ndir;
    return t;
}

int locate_doc_hits_dev(rbg_index *ix, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N, uint64_t max_hits, const void *d_order,
                        uint64_t *d_sets, uint32_t *d_ndocs, uint32_t *d_nodoc, uint64_t *d_doc_reads, uint64_t *d_doc_locs, void *stream) {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    if (!doc_dev_current(ix)) return RBG_ENOTLOADED;
    if (ix->doc_dev.ndocs > kLocDocLdsDocs) return RBG_EARG;   // the table does not fit LDS: plan + fill + rbg_doc_hits_dev
    if (N && (!d_lo || !d_hi || !d_k)) return RBG_EARG;
    if (d_order && N >= 0xFFFFFFFFull) return RBG_EARG;
    // (with every output NULL the walk still runs: rbg_counters sees it)
    return launch_locate_doc_hits(ix->dev, ix->cfg, doc_table_of(ix->doc_dev), d_lo, d_hi, d_k, N, max_hits, d_order, d_sets, d_ndocs, d_nodoc, d_doc_reads,
                                  d_doc_locs, stream) ? RBG_ENODEV : RBG_OK;
}

// rbg_doc_hits walks the batch in chunks so that the device scratch stays bounded.  A CHUNK is at most kDocHitsChunkReads reads (RBG_DOC_HITS_CHUNK overrides):
// it is staged and searched ONCE.  Its locate plan, order, fill and the reduction then go over PIECES of the chunk, each of at most kDocHitsChunkLocs locations
// (RBG_DOC_HITS_CHUNK_LOCS overrides): a piece over the bound is halved and planned again until it fits or is one read, whose locations are then taken whole.
// Only the plan is repeated, which counts nothing: rbg_counters sees every read once and every location once, however the batch is cut.
// THE FUSED PATH (tables of at most kLocDocLdsDocs documents): per chunk stage, search, order and ONE walk that reduces into the sets (rbg_locate_docs.hpp) --
// no plan, no total read back, no pieces, since nothing is stored per location.  The two-step path above stays for larger tables, with
// RBG_DOC_HITS_FUSED=0 (A/B), and whenever RBG_DOC_HITS_CHUNK_LOCS is set: that variable bounds a scratch only the two-step path has.
constexpr uint64_t kDocHitsChunkReads = uint64_t(1) << 21, kDocHitsChunkLocs = uint64_t(1) << 28;
constexpr bool kDocHitsFusedDefault = true;
bool doc_hits_fused(const uint32_t ndocs) {
    if (ndocs > kLocDocLdsDocs) return false;
    const char *locs = std::getenv("RBG_DOC_HITS_CHUNK_LOCS");
    if (locs && *locs) return false;
    const char *e = std::getenv("RBG_DOC_HITS_FUSED");
    return e && *e ? e[0] != '0' : kDocHitsFusedDefault;
}
uint64_t doc_hits_env(const char *name, uint64_t dflt) {
    const char *e = std::getenv(name);
    const long long v = e && *e ? std::atoll(e) : 0;
    return v > 0 ? static_cast<uint64_t>(v) : dflt;
}
}  // namespace

extern "C" {

int rbg_docs_prepare(rbg_index *ix) {
    return guarded([&]() -> int {
    if (!ix) return RBG_EARG;
    return docs_prepare(ix);
    });
}

size_t rbg_doc_hits_words(const rbg_index *ix) {
    if (!ix || !has_docs(ix)) return 0;
    return (ix->H().dl.starts.size() + 63) / 64;
}

int rbg_resolve_offsets_dev(rbg_index *ix, const uint64_t *d_locs, uint64_t M, uint32_t *d_doc, uint64_t *d_offset, void *stream) {
    return guarded([&]() -> int { return resolve_offsets_dev(ix, d_locs, false, M, d_doc, d_offset, stream); });
}

int rbg_resolve_offsets_dev32(rbg_index *ix, const uint32_t *d_locs32, uint64_t M, uint32_t *d_doc, uint64_t *d_offset, void *stream) {
    return guarded([&]() -> int { return resolve_offsets_dev(ix, d_locs32, true, M, d_doc, d_offset, stream); });
}

int rbg_doc_hits_dev(rbg_index *ix, const uint64_t *d_locs, const uint64_t *d_loc_off, uint64_t N, uint64_t *d_sets, uint32_t *d_ndocs, uint32_t *d_nodoc,
                     uint64_t *d_doc_reads, void *stream) {
    return guarded([&]() -> int { return doc_hits_dev(ix, d_locs, false, d_loc_off, N, d_sets, d_ndocs, d_nodoc, d_doc_reads, stream); });
}

int rbg_doc_hits_dev32(rbg_index *ix, const uint32_t *d_locs32, const uint64_t *d_loc_off, uint64_t N, uint64_t *d_sets, uint32_t *d_ndocs,
                       uint32_t *d_nodoc, uint64_t *d_doc_reads, void *stream) {
    return guarded([&]() -> int { return doc_hits_dev(ix, d_locs32, true, d_loc_off, N, d_sets, d_ndocs, d_nodoc, d_doc_reads, stream); });
}

int rbg_locate_doc_hits_dev(rbg_index *ix, const uint64_t *d_lo, const uint64_t *d_hi, const uint64_t *d_k, uint64_t N, uint64_t max_hits, const void *d_order,
                            uint64_t *d_sets, uint32_t *d_ndocs, uint32_t *d_nodoc, uint64_t *d_doc_reads, uint64_t *d_doc_locs, void *stream) {
    return guarded([&]() -> int {
        return locate_doc_hits_dev(ix, d_lo, d_hi, d_k, N, max_hits, d_order, d_sets, d_ndocs, d_nodoc, d_doc_reads, d_doc_locs, stream);
    });
}

int rbg_doc_hits(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t max_hits, uint64_t *lo, uint64_t *hi, uint64_t *sets,
                 uint32_t *ndocs, uint32_t *nodoc, uint64_t *doc_reads) {
    return rbg_doc_hits_locs(ix, seqs, off, N, max_hits, lo, hi, sets, ndocs, nodoc, doc_reads, nullptr);
}

// find_range_w_toehold, the locate plan, order and fill, then the document sets -- chunk by chunk, the locations never leaving the device (as 32-bit values on
// an index with 4-byte positions: rbg_locate_fill_dev32's form).  Per read 16 bytes of range + 8 W bytes of set + 4 (+ 4) bytes of counts come back.
// The fused path: the order, then one walk that writes the sets and counts (above).
int rbg_doc_hits_locs(rbg_index *ix, const uint8_t *seqs, const uint64_t *off, uint64_t N, uint64_t max_hits, uint64_t *lo, uint64_t *hi, uint64_t *sets,
                      uint32_t *ndocs, uint32_t *nodoc, uint64_t *doc_reads, uint64_t *doc_locs) {
    return guarded([&]() -> int {
    if (!queryable(ix)) return RBG_ENODEV;
    if (!ix->H().has_tsa) return RBG_ENOTLOADED;
    int rc;
    if ((rc = docs_prepare(ix))) return rc;
    if (N && (!lo || !hi || !sets || !ndocs)) return RBG_EARG;
    if ((rc = check_offsets(off, N))) return rc;
    if (N && off[N] && !seqs) return RBG_EARG;
    if (N == 0) return RBG_OK;
    DeviceScope scope(ix->device);
    if (scope.rc) return scope.rc;
    hipStream_t st = hipStreamPerThread;
    const rbg_index::DocDev &v = ix->doc_dev;
    const uint64_t W = (v.ndocs + 63) / 64;
    const bool locs32 = ix->H().pos_bytes == 4;
    DevBuf ddr;
    if (doc_reads) {
        if ((rc = ddr.alloc(v.ndocs * 8))) return rc;
        HIP_TRY(hipMemsetAsync(ddr.p, 0, v.ndocs * 8, st));
    }
    DevBuf ddl;
    if (doc_locs) {
        if ((rc = ddl.alloc(v.ndocs * 8))) return rc;
        HIP_TRY(hipMemsetAsync(ddl.p, 0, v.ndocs * 8, st));
    }
    const bool fused = doc_hits_fused(v.ndocs);
    const uint64_t chunk = std::min(N, doc_hits_env("RBG_DOC_HITS_CHUNK", kDocHitsChunkReads));
    const uint64_t max_locs = doc_hits_env("RBG_DOC_HITS_CHUNK_LOCS", kDocHitsChunkLocs);
    std::vector<uint64_t> coff;
    for (uint64_t c0 = 0; c0 < N; c0 += chunk) {
        const uint64_t cn = std::min(chunk, N - c0);
        coff.resize(cn + 1);
        for (uint64_t i = 0; i <= cn; ++i) coff[i] = off[c0 + i] - off[c0];
        ReadBatch rbat;
        if ((rc = rbat.stage(seqs + off[c0], coff.data(), cn, st))) return rc;
        DevBuf dlo, dhi, dk, dloff, dtmp;
        const size_t tmp_bytes = fused ? 0 : scan_tmp_bytes(cn);   // (the plan's scratch: the two-step path's alone)
        if ((rc = dlo.alloc(cn * 8)) || (rc = dhi.alloc(cn * 8)) || (rc = dk.alloc(cn * 8))) return rc;
        if (!fused && ((rc = dloff.alloc((cn + 1) * 8)) || (rc = dtmp.alloc(tmp_bytes)))) return rc;
        if (launch_find_range(ix->dev, ix->cfg, rbat.seqs.as<uint8_t>(), rbat.off.as<uint64_t>(), cn, dlo.as<uint64_t>(), dhi.as<uint64_t>(),
                              dk.as<uint64_t>(), st))
            return RBG_ENODEV;
        // the ranges of the whole chunk leave through the big-copy path, like the sets below
        if ((rc = d2h_result(lo + c0, dlo.p, cn * 8, st)) || (rc = d2h_result(hi + c0, dhi.p, cn * 8, st))) return rc;
        if (fused) {
            DevBuf dord, dsets, dnd, dnod;
            const void *order = nullptr;
            if ((rc = make_order(ix, dk.as<uint64_t>(), cn, dord, st, &order))) return rc;
            if ((rc = dsets.alloc(cn * W * 8)) || (rc = dnd.alloc(cn * 4)) || (rc = dnod.alloc(cn * 4))) return rc;
            if (launch_locate_doc_hits(ix->dev, ix->cfg, doc_table_of(v), dlo.as<uint64_t>(), dhi.as<uint64_t>(), dk.as<uint64_t>(), cn, max_hits, order,
                                       dsets.as<uint64_t>(), dnd.as<uint32_t>(), nodoc ? dnod.as<uint32_t>() : nullptr, doc_reads ? ddr.as<uint64_t>() : nullptr,
                                       doc_locs ? ddl.as<uint64_t>() : nullptr, st))
                return RBG_ENODEV;
            if ((rc = d2h_result(sets + c0 * W, dsets.p, cn * W * 8, st)) || (rc = d2h_result(ndocs + c0, dnd.p, cn * 4, st))) return rc;
            if (nodoc && (rc = d2h_result(nodoc + c0, dnod.p, cn * 4, st))) return rc;
            continue;
        }
        for (uint64_t s0 = 0, sn = cn; s0 < cn; s0 += sn, sn = std::min(cn - s0, 2 * sn)) {   // pieces [s0, s0 + sn) of the chunk; the next one tries twice the reads
            const uint64_t *plo = dlo.as<uint64_t>() + s0, *phi = dhi.as<uint64_t>() + s0, *pk = dk.as<uint64_t>() + s0;
            uint64_t total = 0;
            for (;;) {
                if (launch_locate_plan(ix->dev, ix->cfg, plo, phi, sn, max_hits, dloff.as<uint64_t>(), dtmp.p, tmp_bytes, st)) return RBG_ENODEV;
                HIP_TRY(hipMemcpyAsync(&total, dloff.as<uint64_t>() + sn, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (total <= max_locs || sn == 1) break;
                sn = (sn + 1) / 2;
            }
            DevBuf dord, dlocs, dsets, dnd, dnod;
            const void *order = nullptr;
            if ((rc = make_order(ix, pk, sn, dord, st, &order))) return rc;
            if ((rc = dlocs.alloc(total * (locs32 ? 4 : 8))) || (rc = dsets.alloc(sn * W * 8)) || (rc = dnd.alloc(sn * 4)) || (rc = dnod.alloc(sn * 4))) return rc;
            if (total && launch_locate_fill(ix->dev, ix->cfg, plo, phi, pk, sn, max_hits, dloff.as<uint64_t>(), locs32 ? nullptr : dlocs.as<uint64_t>(), nullptr,
                                            order, st, nullptr, locs32 ? dlocs.as<uint32_t>() : nullptr))
                return RBG_ENODEV;
            if (launch_doc_hits(v.sorted, v.dir, v.size, v.ndocs, v.shift, v.ndir, dlocs.p, locs32, dloff.as<uint64_t>(), sn, dsets.as<uint64_t>(),
                                dnd.as<uint32_t>(), nodoc ? dnod.as<uint32_t>() : nullptr, doc_reads ? ddr.as<uint64_t>() : nullptr, docs_group(), st))
                return RBG_ENODEV;
            if (doc_locs && launch_doc_locs(v.sorted, v.dir, v.size, v.ndocs, v.shift, v.ndir, dlocs.p, locs32, total, ddl.as<uint64_t>(), st)) return RBG_ENODEV;
            const uint64_t r0 = c0 + s0;
            if ((rc = d2h_result(sets + r0 * W, dsets.p, sn * W * 8, st)) || (rc = d2h_result(ndocs + r0, dnd.p, sn * 4, st))) return rc;   // (each blocks until its data has arrived)
            if (nodoc && (rc = d2h_result(nodoc + r0, dnod.p, sn * 4, st))) return rc;
        }
    }
    if (doc_reads) {
        std::vector<uint64_t> add(v.ndocs);
        HIP_TRY(hipMemcpyAsync(add.data(), ddr.p, v.ndocs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t d = 0; d < v.ndocs; ++d) doc_reads[d] += add[d];
    }
    if (doc_locs) {
        std::vector<uint64_t> add(v.ndocs);
        HIP_TRY(hipMemcpyAsync(add.data(), ddl.p, v.ndocs * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t d = 0; d < v.ndocs; ++d) doc_locs[d] += add[d];
    }
    return RBG_OK;
    });
}

}  // extern "C"
