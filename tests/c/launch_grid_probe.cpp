// Prints what csrc/launch_grid.hpp computes, for tests/test_launch_grid.py (a host program: the header includes nothing of HIP).
//   launch_grid_probe blocks <work_items> <threads> <cap>   -> grid_blocks
//   launch_grid_probe for <work_items> <threads> [own_cap]   -> grid_for (reads HEAMD_GRID_CAP)
//   launch_grid_probe for_blocks <items> <threads> [own_cap] -> grid_for_blocks (reads HEAMD_GRID_CAP)
//   launch_grid_probe exact <work_items> <threads>           -> exact_grid
//   launch_grid_probe max <threads>                          -> max_blocks
//   launch_grid_probe fits <blocks> <threads>                -> launch_fits (0 / 1)
// Several queries may follow one another on the command line; one answer per line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "launch_grid.hpp"

static_assert(heamd::launch_grid::max_blocks(256) == 16777215, "256-lane workgroups: 16 777 215 of them");
static_assert(heamd::launch_grid::grid_blocks(SIZE_MAX, 256, SIZE_MAX) == (SIZE_MAX / 256) + 1, "no wrap at the top");

int main(int argc, char** argv) {
    namespace lg = heamd::launch_grid;
    auto number = [&](int i) { return static_cast<size_t>(std::strtoull(argv[i], nullptr, 10)); };
    auto is_number = [&](int i) { return i < argc && argv[i][0] >= '0' && argv[i][0] <= '9'; };
    for (int i = 1; i < argc;) {
        const char* what = argv[i++];
        unsigned long long answer = 0;
        if (std::strcmp(what, "blocks") == 0 && i + 2 < argc) {
            answer = lg::grid_blocks(number(i), static_cast<unsigned>(number(i + 1)), number(i + 2));
            i += 3;
        } else if ((std::strcmp(what, "for") == 0 || std::strcmp(what, "for_blocks") == 0) && i + 1 < argc) {
            const size_t items = number(i);
            const unsigned threads = static_cast<unsigned>(number(i + 1));
            i += 2;
            const bool own = is_number(i);
            const size_t own_cap = own ? number(i++) : SIZE_MAX;
            answer = std::strcmp(what, "for") == 0 ? (own ? lg::grid_for(items, threads, own_cap) : lg::grid_for(items, threads))
                                                   : lg::grid_for_blocks(items, threads, own_cap);
        } else if (std::strcmp(what, "exact") == 0 && i + 1 < argc) {
            answer = lg::exact_grid(number(i), static_cast<unsigned>(number(i + 1)));
            i += 2;
        } else if (std::strcmp(what, "max") == 0 && i < argc) {
            answer = lg::max_blocks(static_cast<unsigned>(number(i)));
            i += 1;
        } else if (std::strcmp(what, "fits") == 0 && i + 1 < argc) {
            answer = lg::launch_fits(number(i), static_cast<unsigned>(number(i + 1))) ? 1 : 0;
            i += 2;
        } else {
            std::fprintf(stderr, "bad query: %s\n", what);
            return 2;
        }
        std::printf("%llu\n", answer);
    }
    return 0;
}
