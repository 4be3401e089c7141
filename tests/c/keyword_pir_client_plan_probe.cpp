// A host program over csrc/keyword_pir_client_plan.hpp (tests/test_keyword_pir_client_reference.py): what the header says about
// a bucket row of E bytes whose replies take R ciphertexts of bpp bytes each.
//   keyword_pir_client_plan_probe R bpp E...
// prints the header's constants "staged_row_limit staged_small_row_limit stage_padding record_bytes max_hash_functions", then per
// E "value_capacity form lds_bytes reply_bytes" (form: 0 staged, 1 direct).
#include <cstdio>
#include <cstdlib>

#include "keyword_pir_client_plan.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    namespace plan = heamd::keyword_pir_client;
    const unsigned long long replies = std::strtoull(argv[1], nullptr, 10), bpp = std::strtoull(argv[2], nullptr, 10);
    std::printf("%llu %llu %llu %llu %u\n", static_cast<unsigned long long>(plan::kStagedRowLimit),
                static_cast<unsigned long long>(plan::kStagedSmallRowLimit), static_cast<unsigned long long>(plan::kStagePadding),
                static_cast<unsigned long long>(plan::kRecordBytes), plan::kMaxHashFunctions);
    for (int i = 3; i < argc; ++i) {
        const plan::Plan p = plan::plan(std::strtoull(argv[i], nullptr, 10), replies, bpp);
        std::printf("%llu %d %llu %llu\n", static_cast<unsigned long long>(p.value_capacity), static_cast<int>(p.form),
                    static_cast<unsigned long long>(p.lds_bytes), static_cast<unsigned long long>(p.reply_bytes));
    }
    return 0;
}
