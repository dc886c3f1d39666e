// rbg_jump.h -- the jump table: for every K-mer (K <= 64) that OCCURS in the text, the search state {lo, hi, toehold} after
// backward search over it.  It is the reference's ftab (rowbowt.hpp:121-131, :726-758) made sparse: the ftab holds every word of
// ftab_k symbols, this table only the words that occur, so K can be four or five times longer.  A read of at least K symbols
// looks up its last K in one probe (usually one 64-byte bucket) instead of the ftab entry and (K - ftab_k) / 8 bucket records;
// a key that is absent -- the read has a symbol in its last K that the text does not -- costs one probe and the read takes the
// ftab path, or ends there when the table is complete (below).  A probe reads whole buckets: the search kernel fetches a bucket as ONE 64-byte request of the owner's quad of lanes (k_runs.hip
// jump_probe_wave) and jump_bucket below settles both of its slots from those sixteen words.  Built at load by the library's own kernels (k_jump.hip), result-neutral by construction.
//
// Key: the K symbols as 2-bit major codes in CONSUMPTION order (symbol t of the key = the read's symbol m - 1 - t at bits
// [2t, 2t + 2) of the 128-bit key; bits from 2K up are zero) -- the layout of the staged reads (rbg_runs_device.hpp) and of the
// packed chunks, so a staged read's key is its first four LDS words, masked.
// Slot: 32 bytes = key (4 words), lo, hi, toehold, tag (1 = occupied, 0 = empty).  A toehold of 2^64 - 1 travels as 0xFFFFFFFF
// (as in the ftab); a word whose toehold fits neither is not inserted.  Two slots per 64-byte bucket; `nb` buckets, open
// addressing over buckets (linear, wrapping at the end).  A probe ends at the matching key or at the first empty slot: the build
// keeps the load at or below one half, so a chain ends soon for absent keys as well.
// Plain C++ (host and device): tests/cpp/jump_table_check.cpp checks the key packing and the probe on a host model of the table.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define RBG_JUMP_HD __host__ __device__ __forceinline__
#else
#define RBG_JUMP_HD inline
#endif

namespace rbg {

constexpr uint32_t kJumpMaxK = 64;     // symbols of a key (128 bits)
constexpr uint32_t kJumpMinK = 16;     // RBG_OPT_JUMP_K: shorter keys would not reach past the ftab
constexpr uint32_t kJumpSlotWords = 8;
constexpr uint32_t kJumpBucketBytes = 64;
constexpr uint32_t kJumpEmptyTag = 0, kJumpFullTag = 1;
constexpr uint32_t kJumpDefaultK = 60;  // RBG_OPT_JUMP_K = -1 (the sweep over 44 / 52 / 60; 60 + 5 x 8 = 100)
// ... built by default only for a replica larger than MI355X's 256 MB last-level cache (below that an index's gathers are cache hits and a
// probe saves nothing; the small indexes of the tests, too, keep today's path unless they ask for the table), and only when the table adds
// at most half of the replica (capi/load.ipp)
constexpr uint64_t kJumpAutoMinBytes = uint64_t(256) << 20;

struct JumpKey {
    uint32_t w[4];
};

// keep the first K symbols of the key (bits [0, 2K)), zero the rest
RBG_JUMP_HD void jump_key_mask(JumpKey &key, uint32_t K) {
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t lo_sym = 16u * i;
        const uint32_t keep = K <= lo_sym ? 0u : (K - lo_sym >= 16u ? 16u : K - lo_sym);
        key.w[i] = keep == 16u ? key.w[i] : (key.w[i] & ((1u << (2u * keep)) - 1u));
    }
}

// symbol t (consumption order) set to the 2-bit code c
RBG_JUMP_HD void jump_key_set(JumpKey &key, uint32_t t, uint32_t c) {
    key.w[t >> 4] |= (c & 3u) << (2u * (t & 15u));
}

RBG_JUMP_HD uint64_t jump_hash(const JumpKey &key) {
    const uint64_t a = key.w[0] | (static_cast<uint64_t>(key.w[1]) << 32);
    const uint64_t b = key.w[2] | (static_cast<uint64_t>(key.w[3]) << 32);
    uint64_t h = (a * 0x9E3779B97F4A7C15ull) ^ ((b + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full);
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 32;
    return h;
}

// the home bucket of a hash among nb (< 2^32) buckets: the high 32 bits scaled to [0, nb)
RBG_JUMP_HD uint64_t jump_home(uint64_t h, uint64_t nb) {
    return ((h >> 32) * nb) >> 32;
}

// One bucket settles a probe.  w = the bucket's 16 words (slot 0, slot 1: key[4], lo, hi, toehold, tag each), read in the probe's order --
// slot 0, then slot 1: kJumpHit0 / kJumpHit1 = the key sits in that slot (v = {lo, hi, toehold}), kJumpAbsent = an empty slot came before a
// match (the chain ends here: the key is not in the table), kJumpNext = both slots hold other keys, the chain goes on in the next bucket.
// Host and device: the kernel fetches a bucket whole (k_runs.hip jump_probe_wave) and decides it here, as jump_probe below does.
constexpr uint32_t kJumpHit0 = 0, kJumpHit1 = 1, kJumpAbsent = 2, kJumpNext = 3;
RBG_JUMP_HD uint32_t jump_bucket(const uint32_t w[16], const JumpKey &key, uint32_t v[3]) {
    for (uint32_t s = 0; s < 2; ++s) {
        const uint32_t *sl = w + kJumpSlotWords * s;
        if (sl[7] == kJumpEmptyTag) return kJumpAbsent;
        if (sl[0] == key.w[0] && sl[1] == key.w[1] && sl[2] == key.w[2] && sl[3] == key.w[3]) {
            v[0] = sl[4]; v[1] = sl[5]; v[2] = sl[6];
            return s;
        }
    }
    return kJumpNext;
}

// the bucket after b in a chain: linear, wrapping at the table's end
RBG_JUMP_HD uint64_t jump_next(uint64_t b, uint64_t nb) { return b + 1 == nb ? 0 : b + 1; }

// The probe.  load(bucket, slot, key_words[4], val_words[4]) reads one slot.  On a hit fills v = {lo, hi, toehold} and returns true;
// `buckets` = buckets read (the STATS count).  At most nb buckets are visited (a table that is never full ends far sooner).
template <typename Load>
RBG_JUMP_HD bool jump_probe(const Load &load, uint64_t nb, const JumpKey &key, uint32_t v[3], uint32_t &buckets) {
    uint64_t b = jump_home(jump_hash(key), nb);
    for (uint64_t step = 0; step < nb; ++step) {
        ++buckets;
        uint32_t w[16];
        load(b, 0, w, w + 4);
        load(b, 1, w + 8, w + 12);
        const uint32_t r = jump_bucket(w, key, v);
        if (r != kJumpNext) return r != kJumpAbsent;
        b = jump_next(b, nb);
    }
    return false;
}

// ---- level 2: a second table, probed after a hit of the first --------------------------------------------------------------------
// The state after K1 + K2 symbols is a function of those symbols alone, but a key holds 64.  `lo` of a non-empty range after K1 symbols
// names that K1-mer uniquely (two different K1-mers have disjoint ranges), so the key of level 2 is {the K2 <= 48 symbols that follow
// the first K1 in consumption order (w[0..2], masked to K2), the parent range's lo (w[3])}: 128 bits again, same slot, same bucket,
// same probe.  Level 2 is a table of its own (DevIndex::jump2_buckets, behind the first in its allocation): its keys never meet a key of level 1.
constexpr uint32_t kJump2MaxK = 48;     // 96 bits of symbols beside the parent's lo
constexpr uint32_t kJump2MinK = 16;
constexpr uint32_t kJump2DefaultK = 40;  // RBG_OPT_JUMP2_K = -1 where level 1 is automatic at K1 = 60: 60 + 40 = 100

// the key of level 2 from three words of symbols (the K2 symbols in consumption order from bit 0; anything above 2 K2 is dropped) and the parent's lo
RBG_JUMP_HD JumpKey jump2_key(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t K2, uint32_t parent_lo) {
    JumpKey key{{s0, s1, s2, 0u}};
    jump_key_mask(key, K2);
    key.w[3] = parent_lo;
    return key;
}

// The K symbols of a read from symbol `from` on, as a key: word(j) = the read's symbols [16 j, 16 j + 16) in consumption order, 2 bits each
// (the staged read's LDS words, a packed chunk's).  Reads words from / 16 .. from / 16 + 4 (the last one only for its low bits; it must
// exist).  from = 0, K = K1: the key of level 1.
template <typename Word>
RBG_JUMP_HD JumpKey jump_key_from_codes(const Word &word, uint32_t from, uint32_t K) {
    const uint32_t w0 = from >> 4, sh = 2u * (from & 15u);
    const uint32_t c0 = word(w0), c1 = word(w0 + 1), c2 = word(w0 + 2), c3 = word(w0 + 3), c4 = word(w0 + 4);
    const auto funnel = [sh](uint32_t lo, uint32_t hi) { return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> sh); };
    JumpKey key{{funnel(c0, c1), funnel(c1, c2), funnel(c2, c3), funnel(c3, c4)}};   // (written out: no array is indexed by a loop variable)
    jump_key_mask(key, K);
    return key;
}

// ... the key of level 2 from a read's codes: the K2 <= 48 symbols from symbol K1 on, and the parent's lo
template <typename Word>
RBG_JUMP_HD JumpKey jump2_key_from_codes(const Word &word, uint32_t K1, uint32_t K2, uint32_t parent_lo) {
    JumpKey key = jump_key_from_codes(word, K1, K2);   // (K2 <= 48: w[3] is masked to zero)
    key.w[3] = parent_lo;
    return key;
}

// ... from a text word (the host model): text[0 .. K1 + K2) as 2-bit codes, the LAST symbol consumed first (backward search), so symbol t of
// the level-2 key is text[K2 - 1 - t] -- the K2 symbols to the left of the K1-mer text[K2 .. K2 + K1)
RBG_JUMP_HD JumpKey jump2_key_from_text(const uint8_t *codes, uint32_t K2, uint32_t parent_lo) {
    JumpKey key{{0, 0, 0, 0}};
    for (uint32_t t = 0; t < K2; ++t) jump_key_set(key, t, codes[K2 - 1 - t]);
    key.w[3] = parent_lo;
    return key;
}

// buckets of a table holding `keys` keys at a load of at most one half (two slots per bucket), at least one
inline uint64_t jump_buckets_for(uint64_t keys) { return keys ? keys : 1; }

// ---- complete levels: an absent key ends the read ---------------------------------------------------------------------------------
// A level is COMPLETE when its build ran to the end (the table stands) and every word of its final enumeration level was inserted.  The
// enumeration (k_jump.hip) holds every word over the major symbols whose range is non-empty, so a complete table lacks a key only when
// the range after that key's symbols is empty: the search may end the read at the probe.  A word the insert skips (a
// toehold the slot cannot express, a range the search found empty), a table that was skipped or declined, a build that stopped early:
// each leaves its level incomplete, and an absent key goes on to the ftab path as before.  The levels are judged apart: a key of level 2
// is probed only after a hit of level 1, and its table is filled from the enumeration alone, whatever level 1 inserted.
constexpr uint32_t kJumpComplete1 = 1u, kJumpComplete2 = 2u;   // DevIndex::jump_complete, rbg_jump_info_t::complete
struct JumpBuilt {
    bool stands;                 // the build ran to the end and its table is the one the index probes
    uint64_t words, inserted;    // words of the final enumeration level; those k_jump_insert counted
};
RBG_JUMP_HD bool jump_level_complete(const JumpBuilt &b) { return b.stands && b.words != 0 && b.inserted == b.words; }
// `absent_ends` = the switch (RBG_JUMP_ABSENT_ENDS, default on): off, no level counts as complete.  Level 2 exists only where level 1 does.
RBG_JUMP_HD uint32_t jump_complete_mask(const JumpBuilt &l1, const JumpBuilt &l2, bool absent_ends) {
    if (!absent_ends || !l1.stands) return 0u;
    return (jump_level_complete(l1) ? kJumpComplete1 : 0u) | (jump_level_complete(l2) ? kJumpComplete2 : 0u);
}
// does an absent key of level `lev` (0, 1) end the read?
RBG_JUMP_HD bool jump_absent_ends(uint32_t mask, uint32_t lev) { return ((mask >> lev) & 1u) != 0; }

}  // namespace rbg
