// Prints what csrc/ciphertext_wire_form.hpp and the 4-byte functions of csrc/serialize_form.hpp choose, for
// tests/test_ciphertext_wire.py (a host program: the headers include nothing of HIP).
//   ciphertext_wire_form_probe ct-serialize   <record_bytes> <record_stride> <records_address>
//   ciphertext_wire_form_probe ct-deserialize <polys> <rows> <log_degree> <record_stride> <records_address>
//   ciphertext_wire_form_probe narrow-serialize   <bytes_address> <rows> <byte_offset>*(rows + 1)
//   ciphertext_wire_form_probe narrow-deserialize <bytes_address> <bytes_per_poly> <rows> <byte_offset>*(rows + 1)
// Several queries may follow one another; one answer per line: "<form> <items per record> <edge free>" for the ct queries,
// "<form>" for the narrow ones.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ciphertext_wire_form.hpp"
#include "serialize_form.hpp"

int main(int argc, char** argv) {
    namespace cf = heamd::ciphertext_wire_form;
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
        if (std::strcmp(what, "ct-serialize") == 0 || std::strcmp(what, "ct-deserialize") == 0) {
            cf::Plan plan{};
            if (what[3] == 's') {
                const uint64_t record_bytes = number();
                const size_t stride = static_cast<size_t>(number());
                plan = cf::for_serialize(record_bytes, stride, static_cast<uintptr_t>(number()));
            } else {
                const uint32_t polys = static_cast<uint32_t>(number()), rows = static_cast<uint32_t>(number());
                const uint32_t log_degree = static_cast<uint32_t>(number());
                const size_t stride = static_cast<size_t>(number());
                plan = cf::for_deserialize(polys, rows, log_degree, stride, static_cast<uintptr_t>(number()));
            }
            if (short_query) break;
            std::printf("%s %llu %d\n", plan.form == cf::Form::kChunk ? "chunk" : "field",
                        static_cast<unsigned long long>(plan.items_per_record), plan.edge_free ? 1 : 0);
        } else if (std::strcmp(what, "narrow-serialize") == 0 || std::strcmp(what, "narrow-deserialize") == 0) {
            const bool deserialize = what[7] == 'd';
            const uintptr_t bytes = static_cast<uintptr_t>(number());
            const size_t bytes_per_poly = deserialize ? static_cast<size_t>(number()) : 0;
            const uint32_t rows = static_cast<uint32_t>(number());
            if (rows > 64) {
                std::fprintf(stderr, "too many rows\n");
                return 2;
            }
            std::vector<uint64_t> byte_offset(rows + 1);
            for (uint64_t& o : byte_offset) o = number();
            if (short_query) break;
            const sf::Form form = deserialize ? sf::for_deserialize_narrow(rows, byte_offset.data(), bytes, bytes_per_poly)
                                              : sf::for_serialize_narrow(rows, byte_offset.data(), bytes);
            std::printf("%s\n", form == sf::Form::kWord ? "word" : "byte");
        } else {
            std::fprintf(stderr, "bad query: %s\n", what);
            return 2;
        }
    }
    if (short_query) {
        std::fprintf(stderr, "short query\n");
        return 2;
    }
    return 0;
}
