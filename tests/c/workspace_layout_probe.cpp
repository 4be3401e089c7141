// workspace_layout_probe.cpp -- csrc/workspace_layout.hpp from a host compiler, for tests/test_workspace_layout.py:
//   <bytes> [<bytes> ...]   one line: the offset add() gave every part in turn, then total()
//   round <bytes>           round16(bytes)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "workspace_layout.hpp"

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "round") == 0) {
        std::printf("%zu\n", heamd::round16(static_cast<size_t>(std::strtoull(argv[2], nullptr, 10))));
        return 0;
    }
    heamd::WorkspaceLayout layout;
    if (layout.total() != 0) return 1;
    for (int i = 1; i < argc; ++i) std::printf("%zu ", layout.add(static_cast<size_t>(std::strtoull(argv[i], nullptr, 10))));
    std::printf("%zu\n", layout.total());
    return 0;
}
