// Host check of rowbowt_amd/csrc/rbg_dispatch.hpp (plain C++17, no HIP): for widths 4 and 8 and both values of one, two and three flags the
// generic lambda receives exactly the matching type and constants -- a static_assert on the tags inside, a counter per combination outside,
// every combination reached once and in the slot its run-time facts name -- and a return value passes through.
// Built with -fsanitize=address,undefined by tests/test_dispatch_host.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "../../rowbowt_amd/csrc/rbg_dispatch.hpp"

using rbg::pos_t;
using rbg::with_flag;
using rbg::with_pos;

template <typename P, bool... F>
struct Combo {   // what a kernel template would be: its own slot per instantiation
    static_assert(std::is_same<P, uint32_t>::value || std::is_same<P, uint64_t>::value, "position types only");
    static int slot() {
        int s = sizeof(P) == 8 ? 1 : 0;
        const bool fs[sizeof...(F) + 1] = {F...};
        for (unsigned t = 0; t < sizeof...(F); ++t) s = 2 * s + (fs[t] ? 1 : 0);
        return s;
    }
};

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

int main() {
    static_assert(std::is_same<pos_t<rbg::pos_tag<uint32_t>>, uint32_t>::value && std::is_same<pos_t<rbg::pos_tag<uint64_t>>, uint64_t>::value, "");
    static_assert(decltype(rbg::yes)::value && !decltype(rbg::no)::value, "");

    // the width alone
    int seen0[2] = {};
    for (const uint32_t bytes : {4u, 8u}) {
        const int got = with_pos(bytes, [&](auto p) {
            using P = pos_t<decltype(p)>;
            static_assert(std::is_same<decltype(p), rbg::pos_tag<uint32_t>>::value || std::is_same<decltype(p), rbg::pos_tag<uint64_t>>::value, "");
            EXPECT(sizeof(P) == bytes);
            ++seen0[Combo<P>::slot()];
            return Combo<P>::slot();
        });
        EXPECT(got == (bytes == 8 ? 1 : 0));
    }
    EXPECT(seen0[0] == 1 && seen0[1] == 1);

    // one, two and three flags under each width
    int seen1[4] = {}, seen2[8] = {}, seen3[16] = {};
    for (const uint32_t bytes : {4u, 8u}) {
        for (int a = 0; a < 2; ++a) {
            const int want1 = (bytes == 8 ? 1 : 0) * 2 + a;
            const int got1 = with_pos(bytes, [&](auto p) { return with_flag(a != 0, [&](auto fa) {
                static_assert(std::is_same<decltype(fa), std::true_type>::value || std::is_same<decltype(fa), std::false_type>::value, "");
                using C = Combo<pos_t<decltype(p)>, decltype(fa)::value>;
                EXPECT(decltype(fa)::value == (a != 0));
                ++seen1[C::slot()];
                return C::slot();
            }); });
            EXPECT(got1 == want1);
            for (int b = 0; b < 2; ++b) {
                const int want2 = want1 * 2 + b;
                const int got2 = with_pos(bytes, [&](auto p) { return with_flag(a != 0, [&](auto fa) { return with_flag(b != 0, [&](auto fb) {
                    using C = Combo<pos_t<decltype(p)>, decltype(fa)::value, decltype(fb)::value>;
                    EXPECT(decltype(fa)::value == (a != 0) && decltype(fb)::value == (b != 0));
                    ++seen2[C::slot()];
                    return C::slot();
                }); }); });
                EXPECT(got2 == want2);
                for (int c = 0; c < 2; ++c) {
                    const int want3 = want2 * 2 + c;
                    const int got3 = with_pos(bytes, [&](auto p) { return with_flag(a != 0, [&](auto fa) { return with_flag(b != 0, [&](auto fb) {
                        return with_flag(c != 0, [&](auto fc) {
                            using C = Combo<pos_t<decltype(p)>, decltype(fa)::value, decltype(fb)::value, decltype(fc)::value>;
                            EXPECT(sizeof(pos_t<decltype(p)>) == bytes);
                            EXPECT(decltype(fa)::value == (a != 0) && decltype(fb)::value == (b != 0) && decltype(fc)::value == (c != 0));
                            ++seen3[C::slot()];
                            return C::slot();
                        });
                    }); }); });
                    EXPECT(got3 == want3);
                }
            }
        }
    }
    for (const int n : seen1) EXPECT(n == 1);
    for (const int n : seen2) EXPECT(n == 1);
    for (const int n : seen3) EXPECT(n == 1);

    // the `yes` / `no` tags in the shape the launchers use them for a subset of the product: a lambda called from an if / else-if chain (this
    // checks the tags, not the launchers: which kernels those instantiate is pinned by tests/golden/kernel_set.json)
    int seen_sub[4] = {};
    for (int fill = 0; fill < 2; ++fill)
        for (int logged = 0; logged < 2; ++logged) {
            auto walk = [&](auto f, auto lg) {
                using C = Combo<uint32_t, decltype(f)::value, decltype(lg)::value>;
                static_assert(!(decltype(f)::value && decltype(lg)::value), "the variant that does not exist is not instantiated");
                ++seen_sub[C::slot()];
                return C::slot();
            };
            const int got = fill ? walk(rbg::yes, rbg::no) : logged ? walk(rbg::no, rbg::yes) : walk(rbg::no, rbg::no);
            EXPECT(got == (fill ? 2 : logged ? 1 : 0));
        }
    EXPECT(seen_sub[0] == 1 && seen_sub[1] == 1 && seen_sub[2] == 2 && seen_sub[3] == 0);

    // return values pass through: a value of another type, a reference, and nothing
    const double d = with_pos(8, [](auto p) { return 0.5 * sizeof(pos_t<decltype(p)>); });
    EXPECT(d == 4.0);
    int target4 = 0, target8 = 0;
    int &ref = with_pos(4, [&](auto p) -> int & { return sizeof(pos_t<decltype(p)>) == 4 ? target4 : target8; });
    ref = 7;
    EXPECT(target4 == 7 && target8 == 0);
    int &ref2 = with_flag(true, [&](auto f) -> int & { return decltype(f)::value ? target8 : target4; });
    EXPECT(&ref2 == &target8);
    with_flag(false, [&](auto f) { target8 = decltype(f)::value ? 1 : 2; });
    EXPECT(target8 == 2);
    // any width other than 4 is the wide one, as ix.pos_bytes == 4 ? ... : ... was
    EXPECT(with_pos(5, [](auto p) { return sizeof(pos_t<decltype(p)>); }) == 8);

    if (fails) return 1;
    std::printf("dispatch ok\n");
    return 0;
}
