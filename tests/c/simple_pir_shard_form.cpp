// Answers questions about csrc/simple_pir_shard_plan.hpp on the host (tests/test_simple_pir_shard_reference.py):
//   form <written> <other> <chunk_size> <bytes>      -> the form's number
//   plan <shard_count> <chunk_size> <length>...      -> error, or "0 total largest per_shard tiles workgroups scratch_bytes"
// one answer per line; `--` separates questions.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simple_pir_shard_plan.hpp"

namespace shard = heamd::simple_pir_shard;

static unsigned long long number(const char* text) { return std::strtoull(text, nullptr, 10); }

int main(int argc, char** argv) {
    int at = 1;
    while (at < argc) {
        int end = at;
        while (end < argc && std::strcmp(argv[end], "--") != 0) ++end;
        const int words = end - at;
        if (words == 5 && std::strcmp(argv[at], "form") == 0) {
            const shard::Form form = shard::form(static_cast<uintptr_t>(number(argv[at + 1])), static_cast<uintptr_t>(number(argv[at + 2])),
                                                 number(argv[at + 3]), number(argv[at + 4]));
            std::printf("%u %u\n", static_cast<unsigned>(form), shard::piece_bytes(form));
        } else if (words >= 3 && std::strcmp(argv[at], "plan") == 0) {
            std::vector<uint64_t> offsets(1, 0);
            for (int i = at + 3; i < end; ++i) offsets.push_back(offsets.back() + number(argv[i]));
            shard::Plan plan;
            const shard::PlanError error = shard::plan(offsets.data(), offsets.size() - 1, number(argv[at + 1]), number(argv[at + 2]), plan);
            if (error != shard::PlanError::kNone) {
                std::printf("%d\n", static_cast<int>(error));
            } else {
                std::printf("0 %llu %llu %llu %zu %zu %zu\n", static_cast<unsigned long long>(plan.total_chunks),
                            static_cast<unsigned long long>(plan.maximum_chunk_count),
                            static_cast<unsigned long long>(plan.chunks_per_shard), plan.map_tiles, plan.count_workgroups,
                            plan.scratch_bytes());
            }
        } else {
            std::fprintf(stderr, "unknown question\n");
            return 2;
        }
        at = end + 1;
    }
    return 0;
}
