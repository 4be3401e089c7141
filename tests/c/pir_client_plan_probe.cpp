// A host program over csrc/pir_client_plan.hpp (tests/test_pir_client_reference.py): the plan of one IndexPirParameter, the
// selection values of its first and last query ciphertext, and the coordinates and position of every index given.
//   pir_client_plan_probe degree t encoding entry_size entry_count indices_count dimension_count dimensions... indices...
// prints "S*I C R per bpp w first last" (a value without an inverse as "-"), then per index "coordinates... position".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pir_client_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 8) return 2;
    std::vector<unsigned long long> args;
    for (int i = 1; i < argc; ++i) args.push_back(std::strtoull(argv[i], nullptr, 10));
    const uint32_t dimension_count = static_cast<uint32_t>(args[6]);
    if (dimension_count == 0 || dimension_count > heamd::pir_client::kMaxDimensions || args.size() < 7 + dimension_count) return 2;
    std::vector<uint32_t> dimensions;
    for (uint32_t k = 0; k < dimension_count; ++k) dimensions.push_back(static_cast<uint32_t>(args[7 + k]));
    const uint64_t t = args[1];
    const heamd::pir_client::Plan plan =
        heamd::pir_client::plan(args[0], t, dimensions.data(), dimension_count, args[4], args[3], args[2] != 0, args[5]);
    std::printf("%llu %llu %llu %llu %llu %llu", static_cast<unsigned long long>(plan.expanded_query_count),
                static_cast<unsigned long long>(plan.query_ciphertexts), static_cast<unsigned long long>(plan.reply_ciphertexts),
                static_cast<unsigned long long>(plan.entries_per_plaintext),
                static_cast<unsigned long long>(plan.bytes_per_plaintext), static_cast<unsigned long long>(plan.width));
    for (uint64_t c : {uint64_t(0), plan.query_ciphertexts - 1}) {
        uint64_t value = 0;
        if (heamd::pir_client::selection_value(heamd::pir_client::input_count(plan, c), t, value))
            std::printf(" %llu", static_cast<unsigned long long>(value));
        else
            std::printf(" -");
    }
    std::printf("\n");
    for (size_t i = 7 + dimension_count; i < args.size(); ++i) {
        uint64_t coordinates[heamd::pir_client::kMaxDimensions];
        heamd::pir_client::coordinates(plan, args[i], coordinates);
        for (uint32_t k = 0; k < dimension_count; ++k) std::printf("%llu ", static_cast<unsigned long long>(coordinates[k]));
        std::printf("%llu\n", static_cast<unsigned long long>(heamd::pir_client::position(plan, args[i])));
    }
    return 0;
}
