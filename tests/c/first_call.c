/* A fresh process's first calls of the six workspace pipelines, over the C ABI alone: no Python, no PyTorch and no HIP call of
 * its own in the process (tests/test_gpu_first_call.py starts one such process per case).
 *
 *   first_call <fixture> <default|cache|workspace> <null|own> <step>...
 *
 * scratch  default: what the library takes when nothing was set;  cache: he_set_scratch_cache(1 GiB) first;  workspace: a caller workspace of exactly the
 *          advertised bytes, filled with 0xA5 bytes.
 * stream   null: the legacy default stream;  own: one from he_stream_create.  Every copy and call goes to that stream.
 * steps    mul relin galois grouped inner dot: one call each, into an output slab of the step's own that was filled with 0x3C
 *          bytes;  `relin` reads the output of the latest `mul` step, or the oracle's product (uploaded) when there was none.
 *          check: read back and compare the outputs of the steps since the last check (this waits for the stream).
 *          settle: wait for the stream and nothing else.
 *          A check is implied at the end.  Every slab is allocated and every copy enqueued before the first step: between two
 *          steps without a check or a settle nothing waits.
 *
 * The fixture (tests/first_call_fixture.py, from seeded inputs and the CPU oracle's outputs) is a stream of uint64 words:
 *   degree, t, moduli_count, moduli[], batch, element,
 *   lhs [batch][2][L][N], rhs [batch][2][L][N]  (adjacent: the grouped call's [2 batch][2][L][N]),
 *   key [L][2][L+1][N], key2 [L][2][L+1][N], secret [L][N],
 *   expected: mul [batch][3][L][N], relin [batch][2][L][N] (of mul and key), galois [batch][2][L][N] (of lhs, element, key),
 *   grouped [2 batch][2][L][N] (lhs under key, rhs under key2), inner [3][L][N] (sum of lhs_i x rhs_i),
 *   dot [batch][L][N] (c0 + c1 s + c2 s^2 of the product), with L = moduli_count - 1.
 *
 * Exit status: 0 every word is the oracle's; 1 a mismatch (evidence on stdout); 2 usage or fixture; 3 a call failed.
 * On a mismatch one run has to be enough to reason from: per step the count of wrong words, the first and last wrong index
 * decoded as (item, polynomial, row, coefficient), the spans of consecutive wrong words and their alignment, and what the wrong
 * words are -- zero, the scratch poison byte or its complement, the output's own fill, the step's input at that position, or
 * something else -- with a few of them printed. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "he_amd.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        int status_ = (call);                                                                         \
        if (status_ != HE_OK) {                                                                       \
            fprintf(stderr, "%s -> %s (%s)\n", #call, he_status_string(status_), he_last_error_message()); \
            return 3;                                                                                 \
        }                                                                                             \
    } while (0)

enum { MUL, RELIN, GALOIS, GROUPED, INNER, DOT, ENTRIES };
static const char* const NAMES[ENTRIES] = {"mul", "relin", "galois", "grouped", "inner", "dot"};
#define OUT_FILL 0x3C
#define MAX_STEPS 16

static he_stream stream;
static uint32_t degree, L;
static size_t batch;

static int upload(uint64_t** device, const uint64_t* host, size_t count) {
    void* raw = NULL;
    int status = he_device_malloc(&raw, count * sizeof(uint64_t));
    if (status != HE_OK) return status;
    *device = (uint64_t*)raw;
    return he_memcpy_h2d(raw, host, count * sizeof(uint64_t), stream);
}
static uint64_t byte_word(unsigned byte) { return 0x0101010101010101ull * (uint64_t)(byte & 0xFF); }

struct step {
    int entry;
    uint64_t* out;            /* device */
    size_t words, polys;      /* [items][polys][L][N] */
    const uint64_t* expected; /* host */
    const uint64_t* input;    /* host: the input slab an output word is formed with at the same (item, poly, row, coefficient) */
    size_t input_polys;
};

static void decode(const struct step* s, size_t index, char* text, size_t size) {
    const size_t coefficient = index % degree, row = index / degree % L, poly = index / ((size_t)degree * L) % s->polys,
                 item = index / ((size_t)degree * L * s->polys);
    snprintf(text, size, "%zu = (item %zu, polynomial %zu, row %zu, coefficient %zu)", index, item, poly, row, coefficient);
}

/* 1 when every word is the oracle's */
static int compare(int number, const struct step* s) {
    uint64_t* back = (uint64_t*)malloc(s->words * sizeof(uint64_t));
    if (he_memcpy_d2h(back, s->out, s->words * sizeof(uint64_t), stream) != HE_OK || he_stream_synchronize(stream) != HE_OK) {
        printf("step %d %s: copy failed (%s)\n", number, NAMES[s->entry], he_last_error_message());
        free(back);
        return 0;
    }
    int poison = -1;
    const char* forced = getenv("HEAMD_SCRATCH_POISON");
    if (forced != NULL && *forced != '\0') poison = (int)strtoul(forced, NULL, 0);
    size_t wrong = 0, first = 0, last = 0, spans = 0, shortest = 0, longest = 0, run = 0, start_bits = 0, printed = 0;
    size_t zero = 0, poisoned = 0, complement = 0, fill = 0, input = 0, other = 0;
    for (size_t i = 0; i <= s->words; ++i) {
        const int bad = i < s->words && back[i] != s->expected[i];
        if (!bad) {
            if (run != 0) {
                shortest = (spans == 1 || run < shortest) ? run : shortest;
                longest = run > longest ? run : longest;
                run = 0;
            }
            continue;
        }
        if (wrong++ == 0) first = i;
        last = i;
        if (run++ == 0) {
            ++spans;
            start_bits |= i;
        }
        /* the step's input at the same place: a polynomial the call adds its update to (none for the polynomials a call forms) */
        const size_t per_item = (size_t)degree * L * s->polys, poly = i / ((size_t)degree * L) % s->polys;
        const uint64_t* at = (s->input != NULL && poly < s->input_polys)
                                 ? s->input + i / per_item * ((size_t)degree * L * s->input_polys) + i % per_item : NULL;
        const char* kind = "other";
        if (back[i] == 0) ++zero, kind = "zero";
        else if (poison >= 0 && back[i] == byte_word((unsigned)poison)) ++poisoned, kind = "poison";
        else if (poison >= 0 && back[i] == byte_word(~(unsigned)poison)) ++complement, kind = "poison complement";
        else if (back[i] == byte_word(OUT_FILL)) ++fill, kind = "output fill (never written)";
        else if (at != NULL && back[i] == *at) ++input, kind = "input at that position";
        else ++other;
        if (printed < 6 && run == 1) {
            char where[160];
            decode(s, i, where, sizeof where);
            printf("step %d %s: word %s is %llu, the oracle says %llu", number, NAMES[s->entry], where, (unsigned long long)back[i],
                   (unsigned long long)s->expected[i]);
            if (at != NULL) printf(", the input there is %llu", (unsigned long long)*at);
            printf(" [%s]\n", kind);
            ++printed;
        }
    }
    free(back);
    if (wrong == 0) {
        printf("step %d %s: ok (%zu words)\n", number, NAMES[s->entry], s->words);
        return 1;
    }
    char a[160], b[160];
    decode(s, first, a, sizeof a);
    decode(s, last, b, sizeof b);
    size_t alignment = 1;
    while (start_bits != 0 && (start_bits & alignment) == 0) alignment <<= 1;
    printf("step %d %s: %zu of %zu words wrong; first %s; last %s\n", number, NAMES[s->entry], wrong, s->words, a, b);
    printf("step %d %s: %zu span(s) of consecutive wrong words, shortest %zu, longest %zu words; every span starts at a multiple of "
           "%zu words (%zu bytes)%s\n", number, NAMES[s->entry], spans, shortest, longest, start_bits == 0 ? s->words : alignment,
           (start_bits == 0 ? s->words : alignment) * 8, (spans == 1 && wrong == last - first + 1) ? "; one contiguous range" : "");
    printf("step %d %s: wrong words that are zero %zu, poison %zu, poison complement %zu, output fill %zu, the input at that position "
           "%zu, something else %zu\n", number, NAMES[s->entry], zero, poisoned, complement, fill, input, other);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    FILE* file = fopen(argv[1], "rb");
    if (file == NULL) return 2;
    fseek(file, 0, SEEK_END);
    const long bytes = ftell(file);
    fseek(file, 0, SEEK_SET);
    uint64_t* words = (uint64_t*)malloc((size_t)bytes);
    if (fread(words, 1, (size_t)bytes, file) != (size_t)bytes) return 2;
    fclose(file);
    const int cache = strcmp(argv[2], "cache") == 0, own_workspace = strcmp(argv[2], "workspace") == 0;
    if (!cache && !own_workspace && strcmp(argv[2], "default") != 0) return 2;
    const int own_stream = strcmp(argv[3], "own") == 0;
    if (!own_stream && strcmp(argv[3], "null") != 0) return 2;

    size_t cursor = 0;
    degree = (uint32_t)words[cursor++];
    const uint64_t t = words[cursor++];
    const uint32_t moduli_count = (uint32_t)words[cursor++];
    const uint64_t* moduli = words + cursor;
    cursor += moduli_count;
    batch = (size_t)words[cursor++];
    const uint64_t element = words[cursor++];
    L = moduli_count - 1;
    const size_t poly = (size_t)L * degree, key_words = (size_t)L * 2 * (L + 1) * degree;
    const size_t sizes[ENTRIES] = {batch * 3 * poly, batch * 2 * poly, batch * 2 * poly, 2 * batch * 2 * poly, 3 * poly, batch * poly};
    const size_t out_polys[ENTRIES] = {3, 2, 2, 2, 3, 1};
    const uint64_t* lhs_host = words + cursor;
    const uint64_t* key_host = lhs_host + 2 * batch * 2 * poly;
    const uint64_t* secret_host = key_host + 2 * key_words;
    const uint64_t* expected[ENTRIES];
    expected[0] = secret_host + poly;
    for (int e = 1; e < ENTRIES; ++e) expected[e] = expected[e - 1] + sizes[e - 1];
    if ((size_t)bytes != (size_t)((const char*)(expected[ENTRIES - 1] + sizes[ENTRIES - 1]) - (const char*)words)) {
        fprintf(stderr, "the fixture has %ld bytes, not those of its header\n", bytes);
        return 2;
    }

    if (cache) CHECK(he_set_scratch_cache((uint64_t)1 << 30));
    he_bfv_context* ctx = NULL;
    CHECK(he_bfv_context_create(degree, t, moduli, moduli_count, &ctx));
    if (he_bfv_ciphertext_moduli_count(ctx) != L) return 2;
    if (own_stream) CHECK(he_stream_create(&stream));

    uint64_t *pair, *keys, *secret, *product;
    CHECK(upload(&pair, lhs_host, 2 * batch * 2 * poly));
    CHECK(upload(&keys, key_host, 2 * key_words));
    CHECK(upload(&secret, secret_host, poly));
    CHECK(upload(&product, expected[MUL], sizes[MUL]));
    const uint64_t *lhs = pair, *rhs = pair + batch * 2 * poly, *key = keys, *key2 = keys + key_words;
    const uint64_t* both[2];
    both[0] = key;
    both[1] = key2;

    const size_t workspace_sizes[ENTRIES] = {
        he_bfv_mul_workspace_bytes(ctx, L, batch),           he_bfv_relinearize_workspace_bytes(ctx, L, batch),
        he_bfv_apply_galois_workspace_bytes(ctx, L, batch),  he_bfv_apply_galois_workspace_bytes(ctx, L, 2 * batch),
        he_bfv_inner_product_workspace_bytes(ctx, L, batch), he_bfv_decrypt_workspace_bytes(ctx, 64, L, 3, 0, batch)};
    /* every step's output slab (0x3C bytes) and workspace (0xA5 bytes) before the first call: between two steps nothing waits */
    struct step steps[MAX_STEPS];
    void* workspaces[MAX_STEPS];
    int count = 0;
    for (int a = 4; a < argc; ++a) {
        int entry = 0;
        while (entry < ENTRIES && strcmp(argv[a], NAMES[entry]) != 0) ++entry;
        if (entry == ENTRIES) {
            if (strcmp(argv[a], "check") != 0 && strcmp(argv[a], "settle") != 0) return 2;
            continue;
        }
        if (count == MAX_STEPS) return 2;
        struct step* s = &steps[count];
        s->entry = entry;
        s->words = sizes[entry];
        s->polys = out_polys[entry];
        s->expected = expected[entry];
        s->input = entry == RELIN ? expected[MUL] : (entry == GALOIS || entry == GROUPED) ? lhs_host : NULL;
        s->input_polys = entry == RELIN ? 3 : 2;
        unsigned char* fill = (unsigned char*)malloc(s->words * 8); /* (pageable: alive until the copy has run) */
        memset(fill, OUT_FILL, s->words * 8);
        CHECK(upload(&s->out, (const uint64_t*)fill, s->words));
        workspaces[count] = NULL;
        if (own_workspace) {
            unsigned char* poison = (unsigned char*)malloc(workspace_sizes[entry]);
            memset(poison, 0xA5, workspace_sizes[entry]);
            CHECK(he_device_malloc(&workspaces[count], workspace_sizes[entry]));
            CHECK(he_memcpy_h2d(workspaces[count], poison, workspace_sizes[entry], stream));
        }
        ++count;
    }

    int next = 0, checked = 0, good = 1;
    const uint64_t* product_now = product;
    for (int a = 4; a <= argc && good; ++a) {
        if (a == argc || strcmp(argv[a], "check") == 0) {
            for (; checked < next; ++checked) good &= compare(checked + 1, &steps[checked]);
            continue;
        }
        if (strcmp(argv[a], "settle") == 0) {
            CHECK(he_stream_synchronize(stream));
            continue;
        }
        struct step* s = &steps[next];
        void* workspace = workspaces[next];
        const size_t workspace_bytes = own_workspace ? workspace_sizes[s->entry] : 0;
        ++next;
        switch (s->entry) {
        case MUL:
            CHECK(he_bfv_mul_device(ctx, L, lhs, rhs, s->out, batch, workspace, workspace_bytes, stream));
            product_now = s->out;
            break;
        case RELIN:
            CHECK(he_bfv_relinearize_device(ctx, L, product_now, key, s->out, batch, workspace, workspace_bytes, stream));
            break;
        case GALOIS:
            CHECK(he_bfv_apply_galois_device(ctx, L, lhs, element, key, s->out, batch, workspace, workspace_bytes, stream));
            break;
        case GROUPED:
            CHECK(he_bfv_apply_galois_grouped_device(ctx, L, lhs, element, both, 2, batch, s->out, workspace, workspace_bytes, stream));
            break;
        case INNER:
            CHECK(he_bfv_inner_product_device(ctx, L, lhs, rhs, batch, s->out, workspace, workspace_bytes, stream));
            break;
        default:
            CHECK(he_bfv_secret_dot_product_device(ctx, 64, L, 3, 0, product, secret, s->out, batch, workspace, workspace_bytes, stream));
        }
    }
    CHECK(he_stream_synchronize(stream));
    if (cache) {
        uint64_t kept = 0;
        CHECK(he_scratch_cached_bytes(&kept));
        if (kept == 0) {
            printf("the block cache kept nothing: the calls took no library scratch\n");
            good = 0;
        }
    }
    he_bfv_context_destroy(ctx);
    if (own_stream) CHECK(he_stream_destroy(stream));
    if (good) printf("first call ok (%d steps)\n", count);
    return good ? 0 : 1;
}
