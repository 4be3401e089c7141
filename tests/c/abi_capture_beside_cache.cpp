// One thread captures a graph in hipStreamCaptureModeGlobal while another takes scratch from the library's block cache through
// misses and evictions: the cache's driver calls (hipMalloc, hipFree, event creation and query) must not be refused, nor
// invalidate the capture.  No Python or PyTorch in the process, so no other allocator disturbs the capture.
//
//   abi_capture_beside_cache <fixture>
//
// The fixture is that of abi_scheme.c (tests/test_abi_c.py writes it): of its words this program reads the head, lhs, rhs, the
// key, the expected ct x ct products (relinearize's input here) and the expected relinearized ciphertexts.
//   thread A  begins a global-mode capture on its stream, enqueues lhs += rhs (he_poly_add_device takes no scratch), waits
//             for B, ends the capture, instantiates and launches the graph
//   thread B  inside A's capture window: six he_bfv_relinearize_device calls with a NULL workspace on its own stream, each
//             into a slab of its own.  After each call it waits for its stream (its capture mode relaxed around the wait only)
//             and calls he_device_trim_scratch(0) in the default mode.
// With he_set_scratch_cache(65536), less than one call's scratch, a call's release is over the limit but still in flight, so
// its block stays cached; after the wait the trim queries it and frees it.  Every call therefore misses (hipMalloc; the first
// one creates the event too) and every block is evicted (hipEventQuery, hipFree) beside the capture.  The program checks both: the block is cached before each trim and nothing is after it.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "he_amd.h"

#define CHECK(call)                                                                                              \
    do {                                                                                                         \
        const int status_ = (call);                                                                              \
        if (status_ != HE_OK) {                                                                                  \
            std::fprintf(stderr, "%s -> %s (%s)\n", #call, he_status_string(status_), he_last_error_message()); \
            return 1;                                                                                            \
        }                                                                                                        \
    } while (0)
#define HIP_CHECK(call)                                                             \
    do {                                                                            \
        const hipError_t error_ = (call);                                           \
        if (error_ != hipSuccess) {                                                 \
            std::fprintf(stderr, "%s -> %s\n", #call, hipGetErrorString(error_)); \
            return 1;                                                               \
        }                                                                           \
    } while (0)

namespace {
constexpr int kCalls = 6;
constexpr uint64_t kBound = 65536;

int upload(uint64_t** device, const uint64_t* host, size_t count) {
    void* raw = nullptr;
    CHECK(he_device_malloc(&raw, count * sizeof(uint64_t)));
    *device = static_cast<uint64_t*>(raw);
    if (host != nullptr) CHECK(he_memcpy_h2d(raw, host, count * sizeof(uint64_t), nullptr));
    return HE_OK;
}
bool same(const char* what, const uint64_t* device, const uint64_t* expected, size_t count) {
    std::vector<uint64_t> back(count);
    if (he_memcpy_d2h(back.data(), device, count * sizeof(uint64_t), nullptr) != HE_OK || he_stream_synchronize(nullptr) != HE_OK) {
        std::fprintf(stderr, "%s: copy failed (%s)\n", what, he_last_error_message());
        return false;
    }
    for (size_t i = 0; i < count; ++i)
        if (back[i] != expected[i]) {
            std::fprintf(stderr, "%s: word %zu is %llu, expected %llu\n", what, i, (unsigned long long)back[i],
                         (unsigned long long)expected[i]);
            return false;
        }
    return true;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* file = std::fopen(argv[1], "rb");
    if (file == nullptr) return 2;
    std::fseek(file, 0, SEEK_END);
    const long bytes = std::ftell(file);
    std::fseek(file, 0, SEEK_SET);
    std::vector<uint64_t> words(static_cast<size_t>(bytes) / sizeof(uint64_t));
    if (std::fread(words.data(), sizeof(uint64_t), words.size(), file) != words.size()) return 2;
    std::fclose(file);
    size_t cursor = 0;
    auto take = [&](size_t count) {
        const uint64_t* at = words.data() + cursor;
        cursor += count;
        return at;
    };
    const uint32_t degree = static_cast<uint32_t>(*take(1));
    const uint64_t t = *take(1);
    const uint32_t moduli_count = static_cast<uint32_t>(*take(1));
    const uint64_t* moduli = take(moduli_count);
    const size_t batch = static_cast<size_t>(*take(1));
    take(1);  // d0
    he_bfv_context* ctx = nullptr;
    CHECK(he_bfv_context_create(degree, t, moduli, moduli_count, &ctx));
    const uint32_t L = he_bfv_ciphertext_moduli_count(ctx);
    const size_t poly = static_cast<size_t>(L) * degree;
    const size_t pair_words = batch * 2 * poly, key_words = static_cast<size_t>(L) * 2 * (L + 1) * degree;

    const uint64_t *lhs_host = take(pair_words), *rhs_host = take(pair_words), *key_host = take(key_words);
    const uint64_t *product_host = take(batch * 3 * poly), *relinearized_host = take(pair_words);
    std::vector<uint64_t> sum_host(pair_words);  // what the graph computes: lhs + rhs, row by row mod q_j
    for (size_t i = 0; i < pair_words; ++i) {
        const uint64_t q = moduli[(i / degree) % L], s = lhs_host[i] + rhs_host[i];
        sum_host[i] = s >= q ? s - q : s;
    }
    uint64_t *lhs, *rhs, *key, *product, *warm, *outs[kCalls];
    CHECK(upload(&lhs, lhs_host, pair_words));
    CHECK(upload(&rhs, rhs_host, pair_words));
    CHECK(upload(&key, key_host, key_words));
    CHECK(upload(&product, product_host, batch * 3 * poly));
    CHECK(upload(&warm, nullptr, pair_words));
    for (uint64_t*& out : outs) CHECK(upload(&out, nullptr, pair_words));
    he_stream stream_a = nullptr, stream_b = nullptr;
    CHECK(he_stream_create(&stream_a));
    CHECK(he_stream_create(&stream_b));
    CHECK(he_stream_synchronize(nullptr));

    // first-use tables and kernel attributes, outside any capture
    CHECK(he_bfv_relinearize_device(ctx, L, product, key, warm, batch, nullptr, 0, stream_b));
    CHECK(he_stream_synchronize(stream_b));
    CHECK(he_poly_add_device(he_bfv_ciphertext_context(ctx, L), warm, warm, batch * 2, stream_a));
    CHECK(he_stream_synchronize(stream_a));
    const uint64_t scratch_bytes = he_bfv_relinearize_workspace_bytes(ctx, L, batch);
    if (scratch_bytes <= kBound) {
        std::fprintf(stderr, "one call's scratch fits the bound: nothing would miss\n");
        return 1;
    }
    CHECK(he_set_scratch_cache(kBound));
    CHECK(he_device_trim_scratch(0));

    std::atomic<int> capturing{0}, b_done{0};  // 0: not yet, 1: yes, -1: failed
    int a_status = 1, b_status = 1;
    std::thread a([&] {
        a_status = [&]() -> int {
            const hipStream_t stream = static_cast<hipStream_t>(stream_a);
            const hipError_t begun = hipStreamBeginCapture(stream, hipStreamCaptureModeGlobal);
            capturing = begun == hipSuccess ? 1 : -1;
            HIP_CHECK(begun);
            const int enqueued = he_poly_add_device(he_bfv_ciphertext_context(ctx, L), lhs, rhs, batch * 2, stream_a);
            while (b_done == 0) std::this_thread::yield();
            hipGraph_t graph = nullptr;
            HIP_CHECK(hipStreamEndCapture(stream, &graph));
            CHECK(enqueued);
            if (graph == nullptr) {
                std::fprintf(stderr, "the capture ended without a graph\n");
                return 1;
            }
            hipGraphExec_t exec = nullptr;
            HIP_CHECK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphLaunch(exec, stream));
            HIP_CHECK(hipStreamSynchronize(stream));
            HIP_CHECK(hipGraphExecDestroy(exec));
            HIP_CHECK(hipGraphDestroy(graph));
            return 0;
        }();
    });
    std::thread b([&] {
        b_status = [&]() -> int {
            while (capturing == 0) std::this_thread::yield();
            if (capturing < 0) return 1;
            for (int k = 0; k < kCalls; ++k) {
                CHECK(he_bfv_relinearize_device(ctx, L, product, key, outs[k], batch, nullptr, 0, stream_b));
                hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
                HIP_CHECK(hipThreadExchangeStreamCaptureMode(&mode));
                const hipError_t waited = hipStreamSynchronize(static_cast<hipStream_t>(stream_b));
                HIP_CHECK(hipThreadExchangeStreamCaptureMode(&mode));
                HIP_CHECK(waited);
                uint64_t held = 0, left = 1;
                CHECK(he_scratch_cached_bytes(&held));
                CHECK(he_device_trim_scratch(0));
                CHECK(he_scratch_cached_bytes(&left));
                if (held < scratch_bytes || left != 0) {  // a hit instead of a miss, or a block the trim could not free
                    std::fprintf(stderr, "call %d: %llu bytes cached before the trim, %llu after\n", k, (unsigned long long)held,
                                 (unsigned long long)left);
                    return 1;
                }
            }
            return 0;
        }();
        b_done = 1;
    });
    a.join();
    b.join();
    if (a_status != 0 || b_status != 0) {
        std::fprintf(stderr, "thread A %s, thread B %s\n", a_status ? "failed" : "ok", b_status ? "failed" : "ok");
        return 1;
    }
    if (!same("the graph's lhs + rhs", lhs, sum_host.data(), pair_words)) return 1;
    for (int k = 0; k < kCalls; ++k)
        if (!same("relinearize beside the capture", outs[k], relinearized_host, pair_words)) return 1;
    uint64_t cached = 0;
    CHECK(he_scratch_cached_bytes(&cached));
    if (cached > kBound) {
        std::fprintf(stderr, "%llu bytes stay cached over a bound of %llu\n", (unsigned long long)cached, (unsigned long long)kBound);
        return 1;
    }
    CHECK(he_set_scratch_cache(0));
    CHECK(he_stream_destroy(stream_a));
    CHECK(he_stream_destroy(stream_b));
    he_bfv_context_destroy(ctx);
    std::printf("capture beside the cache ok (%d calls, %d misses and evictions, %llu bytes cached at the end)\n", kCalls, kCalls,
                (unsigned long long)cached);
    return 0;
}
