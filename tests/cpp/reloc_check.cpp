// reloc_check.cpp -- rbg_reloc_check.hpp on fake records (tests/test_reloc_check_host.py builds this with the host compiler under ASan + UBSan).
// A record with scalars, 32-bit pairs, several pointers and a pointer array is "replicated" by the rule the library follows (copy, then re-point the
// members by hand) over allocation sets of 1, 2 and 40 ranges; the check must find nothing on a correct copy and must name, at its byte offset and with its
// class, each mistake planted on purpose.  The addresses are numbers: nothing is ever dereferenced.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../rowbowt_amd/csrc/rbg_reloc_check.hpp"

using namespace rbg;

namespace {

struct Inner { const void *a; uint64_t f; uint32_t s, t; };
struct Rec {
    uint64_t n, r;
    const void *p0;
    uint32_t u0, u1;          // a pair of 32-bit scalars in one word
    const void *p1;
    uint32_t lone;            // followed by four bytes of padding
    const void *p2;
    const void *arr[8];
    uint64_t big;
    const void *p3;
    uint32_t v0, v1;
};
static_assert(sizeof(Rec) % 8 == 0 && offsetof(Rec, p2) == offsetof(Rec, lone) + 8, "the record has padding, and whole words");

int g_fail = 0;
unsigned long long g_checks = 0;
#define EXPECT(c)                                                                        \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
    } while (0)

const void *at(uint64_t a) { return reinterpret_cast<const void *>(static_cast<uintptr_t>(a)); }
uint64_t num(const void *p) { return static_cast<uint64_t>(reinterpret_cast<uintptr_t>(p)); }

// what the library does to a pointer member
const void *fix(const std::vector<RelocRange> &from, const std::vector<RelocRange> &to, const void *p) {
    if (!p) return nullptr;
    const size_t i = reloc_range_of(from.data(), from.size(), num(p));
    return i == from.size() ? nullptr : at(num(to[i].p) + (num(p) - num(from[i].p)));
}

// allocation sets: `k` source ranges from a device-like base, the targets either far away (another device) or INTERLEAVED with the sources
// (a replica on the same device: every target lies between two sources)
void make_ranges(size_t k, bool interleaved, std::vector<RelocRange> &from, std::vector<RelocRange> &to) {
    from.clear(); to.clear();
    const uint64_t base = 0x7f3a00000000ull, gap = 0x200000;
    for (size_t i = 0; i < k; ++i) {
        const size_t bytes = 0x10000 * (1 + i % 5);
        from.push_back({at(base + 2 * i * gap), bytes});
        to.push_back({at(interleaved ? base + (2 * i + 1) * gap : 0x7e1100000000ull + i * gap), bytes});
    }
}

struct Planted { Rec src; uint64_t nonnull; };
// pointers into range j of `from`, spread over the members; member `arr[7]` and p3 stay null
Planted plant(const std::vector<RelocRange> &from) {
    Planted P;
    std::memset(&P.src, 0, sizeof(Rec));   // (padding equal by construction, as the library guarantees it)
    const size_t k = from.size();
    auto in = [&](size_t j, uint64_t o) { return at(num(from[j % k].p) + o % from[j % k].bytes); };
    Rec &s = P.src;
    s.n = 18000; s.r = 4000; s.u0 = 7; s.u1 = 0xFFFFFFFFu; s.lone = 12; s.big = (uint64_t(1) << 40) - 1; s.v0 = 3; s.v1 = 64;
    s.p0 = in(0, 0);                                   // first byte of an allocation
    s.p1 = in(k - 1, from[(k - 1) % k].bytes - 1);     // last byte of one
    s.p2 = in(k / 2, 4096);
    for (size_t t = 0; t < 7; ++t) s.arr[t] = in(t * 7 + 1, 64 * t);
    s.arr[7] = nullptr;
    s.p3 = nullptr;
    P.nonnull = 3 + 7;
    return P;
}
Rec replicate(const Rec &src, const std::vector<RelocRange> &from, const std::vector<RelocRange> &to) {
    Rec d;
    std::memcpy(&d, &src, sizeof(Rec));
    d.p0 = fix(from, to, d.p0); d.p1 = fix(from, to, d.p1); d.p2 = fix(from, to, d.p2); d.p3 = fix(from, to, d.p3);
    for (auto &p : d.arr) p = fix(from, to, p);
    return d;
}
uint64_t run(const Rec &s, const Rec &d, const std::vector<RelocRange> &from, const std::vector<RelocRange> &to, std::vector<RelocViolation> &v) {
    v.clear();
    return reloc_check(&s, &d, sizeof(Rec), from.data(), to.data(), from.size(), v);
}

}  // namespace

int main() {
    std::vector<RelocRange> from, to;
    std::vector<RelocViolation> v;
    unsigned long long controls = 0;
    for (size_t k : {size_t(1), size_t(2), size_t(40)})
        for (bool interleaved : {false, true}) {
            make_ranges(k, interleaved, from, to);
            const Planted P = plant(from);
            const Rec good = replicate(P.src, from, to);
            // a correct copy: nothing found, every non-null pointer planted is recognised, null stays null and is not counted
            EXPECT(run(P.src, good, from, to, v) == P.nonnull && v.empty());
            EXPECT(good.p3 == nullptr && good.arr[7] == nullptr);
            EXPECT(num(good.p0) == num(to[0].p) && num(good.p1) == num(to[k - 1].p) + to[k - 1].bytes - 1);
            // positive control 1: one pointer left as it was
            for (size_t off : {offsetof(Rec, p0), offsetof(Rec, p1), offsetof(Rec, arr) + 3 * sizeof(void *)}) {
                Rec d = good;
                std::memcpy(reinterpret_cast<char *>(&d) + off, reinterpret_cast<const char *>(&P.src) + off, 8);
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == off && v[0].fault == kRelocStillSource);
                ++controls;
            }
            // positive control 2: a pointer to memory outside every tracked range, which re-pointing nulls
            {
                Rec s = P.src;
                s.p3 = at(0x7f3900000040ull);   // below the first range
                const Rec d = replicate(s, from, to);
                EXPECT(d.p3 == nullptr);
                EXPECT(run(s, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, p3) && v[0].fault == kRelocChanged);
                ++controls;
            }
            // positive control 3: re-pointed, but into the wrong allocation (k >= 2), or to the right one at the wrong offset
            {
                Rec d = good;
                d.p2 = k >= 2 ? at(num(to[(k / 2 + 1) % k].p) + 4096) : at(num(good.p2) + 8);
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, p2) && v[0].fault == kRelocWrongTarget);
                d = good;
                d.arr[6] = nullptr;   // a tracked pointer that became null is "something else" too
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, arr) + 6 * sizeof(void *) && v[0].fault == kRelocWrongTarget);
                ++controls;
            }
            // positive control 4: a scalar changed -- a 64-bit one, one half of a 32-bit pair, and the padding behind `lone`
            {
                Rec d = good;
                d.r += 1;
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, r) && v[0].fault == kRelocChanged);
                d = good;
                d.u1 = 5;
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, u0) && v[0].fault == kRelocChanged);
                d = good;
                reinterpret_cast<unsigned char *>(&d)[offsetof(Rec, lone) + 5] = 0xAA;
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, lone) && v[0].fault == kRelocChanged);
                ++controls;
            }
            // several at once, in offset order
            {
                Rec d = good;
                d.p0 = P.src.p0; d.big = 1; d.arr[0] = at(num(good.arr[0]) + 1);
                EXPECT(run(P.src, d, from, to, v) == P.nonnull && v.size() == 3 && v[0].offset == offsetof(Rec, p0) && v[0].fault == kRelocStillSource &&
                       v[1].offset == offsetof(Rec, arr) && v[1].fault == kRelocWrongTarget && v[2].offset == offsetof(Rec, big) && v[2].fault == kRelocChanged);
            }
            // the ends of an allocation: first and last byte are inside, one past the end is not (and neither is the byte before the first)
            for (size_t j : {size_t(0), k - 1}) {
                const uint64_t b = num(from[j].p), e = b + from[j].bytes;
                EXPECT(reloc_range_of(from.data(), k, b) == j && reloc_range_of(from.data(), k, e - 1) == j);
                EXPECT(reloc_range_of(from.data(), k, e) == k && reloc_range_of(from.data(), k, b - 1) == k);
                Rec s = P.src;
                s.p3 = at(e);   // one past the end: no tracked pointer, so the library nulls it and the check says "changed", not "pointer"
                const Rec d = replicate(s, from, to);
                EXPECT(run(s, d, from, to, v) == P.nonnull && v.size() == 1 && v[0].offset == offsetof(Rec, p3) && v[0].fault == kRelocChanged);
            }
            // a target address is no source pointer: a record that already holds the replica's pointers has none to recognise when the targets are apart
            if (!interleaved) EXPECT(run(good, good, from, to, v) == 0 && v.empty());
        }
    // two allocations adjacent in address: the last byte of the first and the first byte of the second go to their own targets
    {
        from = {{at(0x7f0000100000ull), 0x1000}, {at(0x7f0000101000ull), 0x2000}};
        to = {{at(0x7f0000900000ull), 0x1000}, {at(0x7f0000500000ull), 0x2000}};
        EXPECT(reloc_range_of(from.data(), 2, 0x7f0000100fffull) == 0 && reloc_range_of(from.data(), 2, 0x7f0000101000ull) == 1);
        EXPECT(reloc_range_of(from.data(), 2, 0x7f0000102fffull) == 1 && reloc_range_of(from.data(), 2, 0x7f0000103000ull) == 2);
        Rec s;
        std::memset(&s, 0, sizeof(Rec));
        s.p0 = at(0x7f0000100fffull); s.p1 = at(0x7f0000101000ull); s.p2 = at(0x7f0000102fffull);
        Rec d = replicate(s, from, to);
        EXPECT(num(d.p0) == 0x7f0000900fffull && num(d.p1) == 0x7f0000500000ull && num(d.p2) == 0x7f0000501fffull);
        EXPECT(run(s, d, from, to, v) == 3 && v.empty());
        d.p1 = at(0x7f0000901000ull);   // as if the two were one allocation: continues past the end of the first target
        EXPECT(run(s, d, from, to, v) == 3 && v.size() == 1 && v[0].offset == offsetof(Rec, p1) && v[0].fault == kRelocWrongTarget);
        ++controls;
    }
    // records back to back with a stride (the pointer tables), and a tail shorter than a word
    {
        make_ranges(2, true, from, to);
        std::vector<Inner> s(5), d(5);
        std::memset(s.data(), 0, 5 * sizeof(Inner));
        for (size_t i = 0; i < 5; ++i) { s[i].a = at(num(from[i % 2].p) + 16 * i); s[i].f = 1000 + i; s[i].s = 8; s[i].t = static_cast<uint32_t>(3000 + i); }
        std::memcpy(d.data(), s.data(), 5 * sizeof(Inner));
        for (size_t i = 0; i < 5; ++i) d[i].a = fix(from, to, d[i].a);
        d[3].a = s[3].a;
        uint64_t ptrs = 0;
        v.clear();
        for (size_t i = 0; i < 5; ++i) {
            const size_t first = v.size();
            ptrs += reloc_check(&s[i], &d[i], sizeof(Inner), from.data(), to.data(), 2, v);
            EXPECT((v.size() > first) == (i == 3));
        }
        EXPECT(ptrs == 5 && v.size() == 1 && v[0].offset == offsetof(Inner, a) && v[0].fault == kRelocStillSource);
        unsigned char a[13] = {0}, b[13] = {0};
        v.clear();
        EXPECT(reloc_check(a, b, 13, from.data(), to.data(), 2, v) == 0 && v.empty());
        b[12] = 1;
        EXPECT(reloc_check(a, b, 13, from.data(), to.data(), 2, v) == 0 && v.size() == 1 && v[0].offset == 8 && v[0].fault == kRelocChanged);
        ++controls;
    }
    // no ranges at all: nothing is a pointer
    {
        Rec s;
        std::memset(&s, 0, sizeof(Rec));
        s.p0 = at(0x7f3a00000000ull);
        EXPECT(reloc_check(&s, &s, sizeof(Rec), nullptr, nullptr, 0, v) == 0);
    }
    EXPECT(std::strcmp(reloc_fault_name(kRelocStillSource), "still points into the source") == 0);
    if (g_fail) return 1;
    std::printf("reloc ok checks %llu controls %llu\n", g_checks, controls);
    return 0;
}
