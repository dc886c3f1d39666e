// rbg_docdir.hpp -- the document of a text position: DocList::doc_and_offset_at (doclist.hpp:46-50) over DocList::doc_bounds_rank (:77-79), as
// rbg_resolve_offset (capi/load.ipp) and k_text.hip's doc_of apply it, with a coarse directory in front of the sorted starts so that the common
// lookup is one directory read and a compare or two instead of a binary search (6 to 16 dependent steps).  Host and device share this text; a
// host compiler takes it alone (tests/cpp/docdir_check.cpp drives builder and lookup against a plain count over the starts).
//
// THE RULE.  starts[ndocs] as GIVEN (rbg_set_docs; the order of the .docs file), sorted[] = the same ascending.  size = the LAST start given + 1
// (wrapping at 2^64) -- not the largest: the reference sizes its bit-vector by the last pair it read, doclist.hpp:66.  For a position l:
// q = min(l + 1, size), l + 1 wrapping at 2^64; j = the number of sorted starts < q.  j == 0: no document (the reference indexes doc_names_[-1]
// there).  Otherwise the document is j - 1 -- entry j - 1 of rbg_doc_table -- and the offset is l - sorted[j - 1].
//
// THE DIRECTORY.  Bucket b covers q in [b << shift, (b + 1) << shift); dir[b] = the number of sorted starts < b << shift, for b = 0 .. nb where
// nb = (size >> shift) + 1 buckets hold every q <= size.  So j lies in [dir[b], dir[b + 1]]: j = dir[b] + #{k in [dir[b], dir[b + 1]) : sorted[k] < q}.
// THE SHIFT RULE (doc_dir_shift): the smallest shift with (size >> shift) < kDocDirPerDoc * ndocs.  That bounds the directory -- nb <= 2 ndocs, so
// at most 2 ndocs + 1 entries of 4 bytes -- and, for documents of about equal length (a pangenome: one per haplotype), leaves at most one start in
// most buckets.  A bucket with up to kDocScanMax candidates is scanned; a crowded one (one huge document beside many small ones) is searched by
// bisection within [dir[b], dir[b + 1]).  Whatever the path, the answer is the count above.
#ifndef RBG_DOCDIR_HPP
#define RBG_DOCDIR_HPP
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RBG_DOC_HD __host__ __device__ __forceinline__
#else
#define RBG_DOC_HD inline
#endif

#include <algorithm>
#include <cstdint>
#include <vector>

namespace rbg {

constexpr uint32_t kDocMaxDocs = 1u << 16;     // documents a device table holds (include/rbg.h RBG_DOCS_MAX)
constexpr uint32_t kDocNone = 0xFFFFFFFFu;     // the document of a position that has none
constexpr uint32_t kDocDirPerDoc = 2;          // buckets per document, at most
constexpr uint32_t kDocScanMax = 4;            // candidates of a bucket that are compared one by one; more: bisection
// which path answered (the optional counters of doc_rank: tests assert that every path is reached)
enum { kDocPathDir = 0, kDocPathScan = 1, kDocPathSearch = 2, kDocPathN = 3 };

inline uint64_t doc_list_size(const uint64_t *starts_given, uint64_t ndocs) { return ndocs ? starts_given[ndocs - 1] + 1 : 0; }   // (wraps like the reference's)
inline uint32_t doc_dir_shift(uint64_t size, uint64_t ndocs) {
    uint32_t shift = 0;
    while (shift < 63 && (size >> shift) >= static_cast<uint64_t>(kDocDirPerDoc) * ndocs) ++shift;
    return shift;
}
inline uint64_t doc_dir_buckets(uint64_t size, uint32_t shift) { return (size >> shift) + 1; }

struct DocDir {
    std::vector<uint64_t> sorted;   // [ndocs]
    std::vector<uint32_t> dir;      // [buckets + 1]
    uint64_t size = 0;
    uint32_t shift = 0;
};
// false: no document, or more than kDocMaxDocs
inline bool doc_dir_build(const uint64_t *starts_given, uint64_t ndocs, DocDir &D) {
    if (ndocs == 0 || ndocs > kDocMaxDocs) return false;
    D.sorted.assign(starts_given, starts_given + ndocs);
    std::sort(D.sorted.begin(), D.sorted.end());
    D.size = doc_list_size(starts_given, ndocs);
    D.shift = doc_dir_shift(D.size, ndocs);
    const uint64_t nb = doc_dir_buckets(D.size, D.shift);
    D.dir.resize(nb + 1);
    uint64_t j = 0;
    for (uint64_t b = 0; b <= nb; ++b) {
        if (b > (~uint64_t(0) >> D.shift)) { D.dir[b] = static_cast<uint32_t>(ndocs); continue; }   // (b << shift is 2^64: every start lies below)
        const uint64_t first = b << D.shift;
        while (j < ndocs && D.sorted[j] < first) ++j;
        D.dir[b] = static_cast<uint32_t>(j);
    }
    return true;
}

// j of the rule: the number of sorted starts < min(l + 1, size).  `shift` is the same for every lane of a launch (a kernel argument: the 64-bit
// shift below takes its amount from a scalar register).  path (nullable): kDocPathN counters, one of them incremented.
RBG_DOC_HD uint32_t doc_rank(const uint64_t *sorted, const uint32_t *dir, const uint64_t size, const uint32_t shift, const uint64_t l,
                             unsigned long long *path = nullptr) {
    const uint64_t q = l + 1 > size ? size : l + 1;
    const uint64_t b = q >> shift;
    uint32_t j = dir[b];
    const uint32_t e = dir[b + 1];
    if (e == j) {
        if (path) path[kDocPathDir] += 1;
        return j;
    }
    if (e - j <= kDocScanMax) {
        if (path) path[kDocPathScan] += 1;
        uint32_t c = 0;
        for (uint32_t k = j; k < e; ++k) c += sorted[k] < q ? 1u : 0u;   // (ascending: a prefix of the candidates)
        return j + c;
    }
    if (path) path[kDocPathSearch] += 1;
    uint32_t hi = e;
    while (j < hi) {   // lower_bound(sorted + j, sorted + e, q)
        const uint32_t mid = j + ((hi - j) >> 1);
        if (sorted[mid] < q) j = mid + 1; else hi = mid;
    }
    return j;
}
// the same j for a caller that holds the sorted starts and the size but no directory (rbg_doc_table's view; rowbowt_gpu.hpp resolve_offsets): the rule, by bisection
RBG_DOC_HD uint64_t doc_rank_search(const uint64_t *sorted, const uint64_t ndocs, const uint64_t size, const uint64_t l) {
    const uint64_t q = l + 1 > size ? size : l + 1;
    uint64_t j = 0, hi = ndocs;
    while (j < hi) {
        const uint64_t mid = j + ((hi - j) >> 1);
        if (sorted[mid] < q) j = mid + 1; else hi = mid;
    }
    return j;
}
// document (kDocNone: none) and offset (the position itself when there is no document) of position l
RBG_DOC_HD uint32_t doc_and_offset(const uint64_t *sorted, const uint32_t *dir, const uint64_t size, const uint32_t shift, const uint64_t l, uint64_t *offset,
                                   unsigned long long *path = nullptr) {
    const uint32_t j = doc_rank(sorted, dir, size, shift, l, path);
    *offset = j ? l - sorted[j - 1] : l;
    return j ? j - 1 : kDocNone;
}

}  // namespace rbg
#endif
