// simple_pir_client_plan_probe.cpp -- csrc/simple_pir_client_plan.hpp from a host compiler, for tests/test_simple_pir_client_reference.py:
//   plan <plaintext_bits> <ciphertext_bits> <N> <word_bits> <entry_count> <entry_size_in_bytes> <entry_size_in_scalar>
//        <entries_per_column> <chunks_per_entry> <database_columns> <column_size> <a_poly_count> <modulus> <std_dev> <batch>
//        <forced_row_block>                     one line: the plan's fields in the order printed below, or "-"
//   fold <p>                                    fold_terms(p)
//   divide <p> <c> <x>...                       divide_and_round(x) for every x, one per line
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "simple_pir_client_plan.hpp"

namespace client = heamd::simple_pir_client;

static unsigned long long number(const char* text) { return std::strtoull(text, nullptr, 10); }

int main(int argc, char** argv) {
    if (argc >= 2 && std::strcmp(argv[1], "plan") == 0 && argc == 18) {
        client::Shape s;
        s.plaintext_bits = static_cast<uint32_t>(number(argv[2]));
        s.ciphertext_bits = static_cast<uint32_t>(number(argv[3]));
        s.lattice_dimension = static_cast<uint32_t>(number(argv[4]));
        s.word_bits = static_cast<uint32_t>(number(argv[5]));
        s.entry_count = number(argv[6]);
        s.entry_size_in_bytes = number(argv[7]);
        s.entry_size_in_scalar = number(argv[8]);
        s.entries_per_column = number(argv[9]);
        s.chunks_per_entry = number(argv[10]);
        s.database_columns = number(argv[11]);
        s.column_size = number(argv[12]);
        s.a_poly_count = number(argv[13]);
        s.modulus = number(argv[14]);
        client::Plan p;
        if (!client::plan(s, static_cast<int>(number(argv[15])), number(argv[16]), number(argv[17]), p)) {
            std::printf("-\n");
            return 0;
        }
        std::printf("%zu %zu %zu %u %u %u %llu %zu %u %llu %zu %zu %zu %zu %zu %zu %zu\n", p.chunk_size, p.query_words, p.result_words,
                    p.sampler.k, p.sampler.words_per_side, p.sampler.stream_bytes,
                    static_cast<unsigned long long>(p.sampler.last_word_mask), p.error_chunks, p.secret_rows_per_pass,
                    static_cast<unsigned long long>(p.fold_terms), p.row_block, p.hint_product_lds_bytes, p.a_polynomials_bytes(),
                    p.encrypt_zero_bytes(), p.codes_bytes, p.precompute_bytes(), p.coefficients_bytes);
        return 0;
    }
    if (argc == 3 && std::strcmp(argv[1], "fold") == 0) {
        std::printf("%llu\n", static_cast<unsigned long long>(client::fold_terms(number(argv[2]))));
        return 0;
    }
    if (argc >= 4 && std::strcmp(argv[1], "divide") == 0) {
        const client::Division d = client::division_for(number(argv[2]), static_cast<uint32_t>(number(argv[3])));
        for (int i = 4; i < argc; ++i)
            std::printf("%llu\n", static_cast<unsigned long long>(client::divide_and_round(number(argv[i]), d)));
        return 0;
    }
    std::fprintf(stderr, "usage: plan ... | fold <p> | divide <p> <c> <x>...\n");
    return 2;
}
