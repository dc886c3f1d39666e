// lmem_shim_check -- prints every call rowbowt_gpu.hpp's get_markers_lmems makes of its callback (rowbowt.hpp:341-404), one
// line per call: "<lo> <hi> <q.first> <q.second> <markers...>", and "end" after each query.
//   lmem_shim_check <index_prefix> <queries, one per line> <wsize> <max_range> [noft]
// The index is loaded with the marker array and, unless `noft`, its .ftab (LoadRbwtFlag::FT, as rb_markers --ftab does).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "rowbowt_gpu.hpp"

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: lmem_shim_check <prefix> <queries> <wsize> <max_range> [noft]\n");
        return 2;
    }
    const bool ft = !(argc > 5 && std::string(argv[5]) == "noft");
    auto flag = rbwt::LoadRbwtFlag::MA;
    if (ft) flag = flag | rbwt::LoadRbwtFlag::FT;
    auto rb = rbwt::load_rowbowt<>(argv[1], flag);
    const uint64_t wsize = std::strtoull(argv[3], nullptr, 10), max_range = std::strtoull(argv[4], nullptr, 10);
    std::ifstream in(argv[2]);
    std::string q;
    while (std::getline(in, q)) {
        rb.get_markers_lmems(q, wsize, max_range, [](std::pair<uint64_t, uint64_t> r, std::pair<size_t, size_t> qp, std::vector<MarkerT> mbuf) {
            std::printf("%llu %llu %llu %llu", static_cast<unsigned long long>(r.first), static_cast<unsigned long long>(r.second),
                        static_cast<unsigned long long>(qp.first), static_cast<unsigned long long>(qp.second));
            for (const MarkerT m : mbuf) std::printf(" %llu", static_cast<unsigned long long>(m));
            std::printf("\n");
        });
        std::printf("end\n");
    }
    return 0;
}
