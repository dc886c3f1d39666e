// rbg_dispatch.hpp -- from a launcher's run-time facts to a kernel's template arguments.  Plain C++17, no HIP: tests/cpp/dispatch_check.cpp
// compiles it with g++ alone.
//
// A kernel template takes the position width as a type (uint32_t / uint64_t) and its variants as bools; a launcher knows the width as
// ix.pos_bytes and the variants as run-time flags.  with_pos and with_flag turn one such fact into a tag and hand it to a generic lambda, which
// names the kernel ONCE and reads the template arguments off the tags' types:
//
//     return with_pos(ix.pos_bytes, [&](auto p) { return with_flag(ssamp != nullptr, [&](auto toe) {
//         return launch_kmer(k_find_range_packed<pos_t<decltype(p)>, decltype(toe)::value>, ...);
//     }); });
//
// Nesting instantiates the whole product of the nested facts.  A launcher whose kernel exists for a SUBSET of its flags must not nest them: it
// writes a generic lambda over the tags and an if / else-if chain that calls it with `yes` and `no`, one call per variant that exists
// (launch_marker_seeds_runs), or folds a flag away with a constexpr condition on the width (launch_locate_fill's HI8).  A variant that is named
// nowhere is not compiled, not linked and not checked by tools/check_isa.py; tests/golden/kernel_set.json pins the set.
#pragma once

#include <cstdint>
#include <type_traits>

namespace rbg {

template <typename T>
struct pos_tag {
    using type = T;
};
template <typename Tag>
using pos_t = typename Tag::type;

constexpr std::true_type yes{};
constexpr std::false_type no{};

// f(pos_tag<uint32_t>{}) at 4-byte positions, f(pos_tag<uint64_t>{}) otherwise; both calls must return the same type
template <typename F>
decltype(auto) with_pos(const uint32_t pos_bytes, F &&f) {
    if (pos_bytes == 4) return f(pos_tag<uint32_t>{});
    return f(pos_tag<uint64_t>{});
}

// f(std::true_type{}) or f(std::false_type{})
template <typename F>
decltype(auto) with_flag(const bool b, F &&f) {
    if (b) return f(yes);
    return f(no);
}

}  // namespace rbg
