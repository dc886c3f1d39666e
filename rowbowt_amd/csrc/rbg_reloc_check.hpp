// rbg_reloc_check.hpp -- what a correctly re-pointed copy of a record looks like, as a check (capi/replicas.ipp replicate_finish applies it to DevIndex and
// to every record of every pointer table; rbg_replica_pointer_check reports its counts).  Plain host C++: tests/cpp/reloc_check.cpp drives it alone.
//
// A replica copies every device allocation of its source -- from[i] becomes to[i], index for index -- and then re-points the records that hold device
// pointers.  Seen as aligned 8-byte words, the source's image of such a record and the replica's must then obey two rules:
//   * a source word that is an address inside from[i] is, on the replica, exactly to[i].p plus the same offset;
//   * every other word is bit-identical.
// Whatever breaks a rule is one of three things, named below: a pointer nobody re-pointed (it still reads the SOURCE's memory: right answers, over the
// peer link), a re-pointed pointer that landed somewhere else, or a word that was no tracked pointer and changed all the same -- in practice a pointer to an
// array that no load path tracked, which re-pointing turns into nullptr ("feature absent": right answers again, by the slow path).
//
// The check does not know which words are pointers: it recognises them by value.  That cannot misfire on the scalars of these records: the 64-bit ones (n, r,
// F, counts, offsets, bucket numbers) are bounded by the index length, below 2^48 and in practice below 2^40, while a device allocation is mapped at the top of
// the 47-bit user address space (0x7f.. in the upper 16 bits); two neighbouring 32-bit scalars read as one word would need an upper half of at least 0x7000'0000 beside
// a lower half that happens to fall into a tracked range of the same 4 GiB -- shifts, depths, flags and K are below 2^8, the counts that may be large
// (nruns, record strides) sit beside small ones.  Were one ever recognised, the check would report "still points into the source" for it, once, on stderr: a
// false alarm to read, never a wrong answer, since nothing is re-pointed on the check's word.
// Padding bytes are compared like any others, so both images must have equal padding BY CONSTRUCTION: the caller makes the replica's record a memcpy of the
// source's before re-pointing its members (replicate_finish), or both are byte copies of the same device memory (the pointer tables).
#ifndef RBG_RELOC_CHECK_HPP
#define RBG_RELOC_CHECK_HPP

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rbg {

struct RelocRange {
    const void *p;
    size_t bytes;
};

enum RelocFault : uint32_t {
    kRelocStillSource = 1,   // a tracked pointer, bit-identical on the replica: a forgotten fix
    kRelocWrongTarget = 2,   // a tracked pointer that became something other than to[i].p + offset
    kRelocChanged = 3,       // not a tracked pointer, yet the replica's word differs (a pointer to untracked memory that was nulled)
};
inline const char *reloc_fault_name(uint32_t f) {
    switch (f) {
        case kRelocStillSource: return "still points into the source";
        case kRelocWrongTarget: return "was a tracked pointer, is something else";
        case kRelocChanged: return "was not a tracked pointer, yet changed";
    }
    return "?";
}

struct RelocViolation {
    size_t offset;    // byte offset of the word in the record
    uint32_t fault;   // RelocFault
};

// index of the range of `r` (n of them) that holds address `a`, or n.  [p, p + bytes): the last byte is inside, one past the end is not.
inline size_t reloc_range_of(const RelocRange *r, size_t n, uint64_t a) {
    for (size_t i = 0; i < n; ++i) {
        const uint64_t b = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(r[i].p));
        if (a >= b && a - b < r[i].bytes) return i;
    }
    return n;
}

// `src` and `dst`: the two images of one record, `bytes` long (the words of a tail shorter than 8 bytes are compared as bytes: "changed" at the tail's offset).
// Appends the violations to `out`; returns the number of words recognised as pointers into from[].
inline uint64_t reloc_check(const void *src, const void *dst, size_t bytes, const RelocRange *from, const RelocRange *to, size_t nranges,
                            std::vector<RelocViolation> &out) {
    const unsigned char *s = static_cast<const unsigned char *>(src), *d = static_cast<const unsigned char *>(dst);
    uint64_t pointers = 0;
    size_t o = 0;
    for (; o + 8 <= bytes; o += 8) {
        uint64_t a, b;
        std::memcpy(&a, s + o, 8);
        std::memcpy(&b, d + o, 8);
        const size_t i = a ? reloc_range_of(from, nranges, a) : nranges;   // (null is no pointer: it stays null and is not counted)
        if (i == nranges) {
            if (a != b) out.push_back({o, kRelocChanged});
            continue;
        }
        ++pointers;
        const uint64_t want = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(to[i].p)) + (a - static_cast<uint64_t>(reinterpret_cast<uintptr_t>(from[i].p)));
        if (b == want) continue;   // (a replica whose to[i] IS from[i] would pass here: replicate_begin always allocates anew)
        out.push_back({o, b == a ? kRelocStillSource : kRelocWrongTarget});
    }
    if (o < bytes && std::memcmp(s + o, d + o, bytes - o) != 0) out.push_back({o, kRelocChanged});
    return pointers;
}

}  // namespace rbg
#endif
