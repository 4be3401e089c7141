// Prints what csrc/serialize_form.hpp chooses, for tests/test_wire_format_reference.py (a host program: the header includes
// nothing of HIP).
//   serialize_form_probe serialize   <log_degree> <bytes_address> <slab_address> <rows> <width>*rows <byte_offset>*(rows + 1)
//   serialize_form_probe deserialize <log_degree> <bytes_address> <slab_address> <bytes_per_poly> <rows> <width>*rows
//                                    <byte_offset>*(rows + 1)
// Several queries may follow one another on the command line; one answer per line: byte, word or tile.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "serialize_form.hpp"

int main(int argc, char** argv) {
    namespace sf = heamd::serialize_form;
    int i = 1;
    bool short_query = false;
    auto number = [&]() -> unsigned long long {
        if (i >= argc) {
            short_query = true;
            return 0;
        }
        return std::strtoull(argv[i++], nullptr, 10);
    };
    while (i < argc) {
        const char* what = argv[i++];
        const bool deserialize = std::strcmp(what, "deserialize") == 0;
        if (!deserialize && std::strcmp(what, "serialize") != 0) {
            std::fprintf(stderr, "bad query: %s\n", what);
            return 2;
        }
        const uint32_t log_degree = static_cast<uint32_t>(number());
        const uintptr_t bytes = static_cast<uintptr_t>(number()), slab = static_cast<uintptr_t>(number());
        const size_t bytes_per_poly = deserialize ? static_cast<size_t>(number()) : 0;
        const uint32_t rows = static_cast<uint32_t>(number());
        if (rows > 64) {
            std::fprintf(stderr, "too many rows\n");
            return 2;
        }
        std::vector<uint32_t> width(rows);
        std::vector<uint64_t> byte_offset(rows + 1);
        for (uint32_t& w : width) w = static_cast<uint32_t>(number());
        for (uint64_t& o : byte_offset) o = number();
        if (short_query) {
            std::fprintf(stderr, "short query: %s\n", what);
            return 2;
        }
        const sf::Form form = deserialize ? sf::for_deserialize(rows, width.data(), byte_offset.data(), bytes, slab, log_degree,
                                                                bytes_per_poly)
                                          : sf::for_serialize(rows, width.data(), byte_offset.data(), bytes, slab, log_degree);
        std::printf("%s\n", form == sf::Form::kTile ? "tile" : form == sf::Form::kWord ? "word" : "byte");
    }
    return 0;
}
