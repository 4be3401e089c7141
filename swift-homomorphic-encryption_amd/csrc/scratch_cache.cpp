// scratch_cache.cpp -- stream-ordered scratch (api_internal.hpp scratch_allocate / scratch_release / scratch_forget_stream) and
// the three entries of include/he_amd.h that steer it.
// Two sources, per device:
//  * the library's own stream-ordered block cache: blocks from hipMalloc, kept on a free list with the stream they were
//    released on and an event recorded there.  A later request on the SAME stream takes a block without any driver call
//    (stream order makes it safe); a request on another stream first makes that stream wait for the block's event.
//    he_set_scratch_cache(bytes) is how much released scratch it may KEEP: 0, the default, and a block goes back to the driver
//    (hipFree) at the first release or trim after its own release has completed -- a call of the same shape on the same
//    stream still gets it back before that;
//  * a HIP memory pool the library creates (release threshold 0), only while the stream is being captured into a graph
//    (allocation and free become graph nodes).
// The pool was the default source until a process's calls were seen to return wrong words with it (tests/c/first_call.c,
// profiles/first_call_matrix.txt): release threshold 0 hands the pool's memory back to the driver at every synchronisation, the
// next request maps memory anew, and the kernels that first wrote such a block had their words replaced by zeros -- a block
// from hipMalloc has never shown that.  Nor does a high release threshold help the pool: hipFreeAsync of ROCm 7.2 holds the
// calling thread until the work enqueued before the PREVIOUS release of that block has finished (bench_tools/pool_probe.hip,
// profiles/r06b_pool_probe.txt: 106 ms kernels, every free from the second cycle on returns after 106 ms).
//
// scratch_ledger.hpp keeps the books and makes every decision; this file makes the driver calls.  Every function has one
// shape: lock, ask the ledger, unlock, act, and where needed lock again to record the outcome.  The one driver call made under
// the mutex is the hipStreamWaitEvent of a hit on another stream's block (enqueue-only on the caller's stream; it has to come
// before the block's event can become a spare one).  A release records its event with the mutex released: block and event are
// that call's alone until they are cached.  Whatever may wait for the device or is refused while another thread captures in
// hipStreamCaptureModeGlobal -- hipMalloc, hipFree, hipEventCreateWithFlags, hipEventQuery, hipStreamSynchronize, the
// hipMemPool calls -- runs with the mutex released, inside a RelaxedCapture.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "api_internal.hpp"
#include "scratch_ledger.hpp"

using heamd::invalid_argument;
using heamd::RelaxedCapture;
using heamd::ScratchLedger;

namespace {
constexpr int kMaxDevices = 64;
struct ScratchState {
    std::mutex mutex;  // guards ledger and limit
    ScratchLedger ledger;
    uint64_t limit = 0;  // he_set_scratch_cache: bytes of released scratch the block cache may keep
    // the device's HIP pool, made at the first request under capture; nullptr after that: the creation was refused (it is not
    // tried again) and such scratch comes from the default pool, untouched
    std::once_flag pool_once;
    std::atomic<hipMemPool_t> pool{nullptr};
};
ScratchState& scratch_state(int device) {
    static ScratchState* states = new ScratchState[kMaxDevices];  // never destroyed: HIP may already be gone at exit
    return states[device];
}
bool current_device(int* device) {
    return hipGetDevice(device) == hipSuccess && *device >= 0 && *device < kMaxDevices;
}
hipEvent_t as_event(ScratchLedger::Handle handle) { return static_cast<hipEvent_t>(handle); }

// (without the mutex) the device's HIP pool, or nullptr
hipMemPool_t hip_pool(ScratchState& state, int device) {
    std::call_once(state.pool_once, [&] {
        RelaxedCapture relaxed;
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) == hipSuccess && pool != nullptr) {
            uint64_t threshold = 0;
            (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &threshold);
            state.pool = pool;
        }
        (void)hipGetLastError();
    });
    return state.pool;
}
bool stream_is_capturing(hipStream_t stream) {
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &capture) != hipSuccess) {
        (void)hipGetLastError();  // the legacy default stream cannot be queried -- nor captured
        return false;
    }
    return capture != hipStreamCaptureStatusNone;
}
// (without the mutex) gives cached blocks whose release has completed back to the driver, oldest first, until at most `keep`
// bytes stay cached; blocks still in flight stay.  One query per cached block.  hipFree may wait for the device: only trims,
// over-limit releases and a hipMalloc out of memory come here.
void evict(ScratchState& state, size_t keep) {
    std::vector<ScratchLedger::Block> blocks;
    {
        std::lock_guard<std::mutex> lock(state.mutex);
        if (state.ledger.cached_bytes() <= keep) return;
        blocks = state.ledger.cached();
    }
    RelaxedCapture relaxed;
    // A block taken meanwhile may have its event recorded anew by now; its tick is then no longer in the ledger and the answer
    // about it counts for nothing.
    std::vector<uint64_t> completed;
    for (const ScratchLedger::Block& block : blocks) {
        if (hipEventQuery(as_event(block.event)) == hipSuccess) completed.push_back(block.tick);
        else (void)hipGetLastError();
    }
    {
        std::lock_guard<std::mutex> lock(state.mutex);
        blocks = state.ledger.evict(keep, completed);
    }
    for (const ScratchLedger::Block& block : blocks) (void)hipFree(block.ptr);
}
// takes `ptr` back into `state`'s cache if it was lent from it
bool release_into(ScratchState& state, void* ptr, hipStream_t stream) {
    size_t bytes = 0, limit = 0;
    hipEvent_t event = nullptr;
    {
        std::lock_guard<std::mutex> lock(state.mutex);
        bytes = state.ledger.reclaim(ptr);
        if (bytes == 0) return false;
        event = as_event(state.ledger.take_spare_event());
    }
    if (event == nullptr) {
        RelaxedCapture relaxed;
        if (hipEventCreateWithFlags(&event, hipEventDisableTiming) != hipSuccess) event = nullptr;
    }
    // (the block and the event are this call's alone until they are cached)
    if (event == nullptr || hipEventRecord(event, stream) != hipSuccess) {
        // no way to tell when the block is free again: wait for the stream, then hand it back
        (void)hipGetLastError();
        {
            RelaxedCapture relaxed;
            (void)hipStreamSynchronize(stream);
            (void)hipFree(ptr);
        }
        if (event != nullptr) {
            std::lock_guard<std::mutex> lock(state.mutex);
            state.ledger.give_spare_event(event);
        }
        return true;
    }
    {
        std::lock_guard<std::mutex> lock(state.mutex);
        state.ledger.cache(ptr, bytes, stream, event);
        limit = static_cast<size_t>(state.limit);
    }
    evict(state, limit);
    return true;
}

// HEAMD_SCRATCH_POISON=<0..255>, a test switch (tests/test_gpu_scratch_poison.py, tests/test_gpu_first_call.py): every block
// is filled with that byte on the requesting stream before its caller sees it and with the complement byte on the releasing
// stream before it is cached or freed.  A kernel that reads scratch it did not write, and work on a side lane that outlives
// the release, then compute from words above every modulus instead of from what the last call left.  Read at each call; unset,
// empty or not such a number: nothing here runs but the getenv.  These are the block cache's blocks: while a stream is being
// captured, the only time the pool lends, nothing is filled (the fills would become nodes of the caller's graph).
int poison_byte() {
    const char* forced = std::getenv("HEAMD_SCRATCH_POISON");
    if (forced == nullptr || *forced == '\0') return -1;
    char* end = nullptr;
    const unsigned long value = std::strtoul(forced, &end, 0);
    return *end != '\0' || value > 255 ? -1 : static_cast<int>(value);
}
// the bytes asked for per block lent while the switch was on: a release has only the pointer
struct PoisonedBlocks {
    std::mutex mutex;
    std::unordered_map<void*, size_t> bytes;
    std::atomic<size_t> lent{0};  // bytes.size(): zero in every process that never set the switch, read without the mutex
};
PoisonedBlocks& poisoned_blocks() {
    static PoisonedBlocks* blocks = new PoisonedBlocks;  // never destroyed, as the states above
    return *blocks;
}
hipError_t poison_lent(void* ptr, size_t bytes, hipStream_t stream, int byte) {
    if (stream_is_capturing(stream)) return hipSuccess;
    {
        PoisonedBlocks& blocks = poisoned_blocks();
        std::lock_guard<std::mutex> lock(blocks.mutex);
        blocks.bytes[ptr] = bytes;
        blocks.lent = blocks.bytes.size();
    }
    return hipMemsetAsync(ptr, byte, bytes, stream);
}
void poison_released(void* ptr, hipStream_t stream) {
    size_t bytes = 0;
    {
        PoisonedBlocks& blocks = poisoned_blocks();
        std::lock_guard<std::mutex> lock(blocks.mutex);
        auto it = blocks.bytes.find(ptr);
        if (it == blocks.bytes.end()) return;  // lent while the switch was off
        bytes = it->second;
        blocks.bytes.erase(it);
        blocks.lent = blocks.bytes.size();
    }
    const int byte = poison_byte();
    if (byte < 0 || stream_is_capturing(stream)) return;
    if (hipMemsetAsync(ptr, ~byte & 0xFF, bytes, stream) != hipSuccess) (void)hipGetLastError();
}

// a block of `bytes` from the source in charge
hipError_t allocate_block(void** out, size_t bytes, hipStream_t stream);
}  // namespace

// he_stream_destroy, the device group, a context's side lanes: a later stream may get the same handle -- the blocks released on
// this one no longer count as released on "the same stream" (their events still order them)
void heamd::scratch_forget_stream(hipStream_t stream) {
    if (stream == nullptr) return;
    int device = 0;
    if (!current_device(&device)) return;
    ScratchState& state = scratch_state(device);
    std::lock_guard<std::mutex> lock(state.mutex);
    state.ledger.forget_stream(stream);
}

hipError_t heamd::scratch_allocate(void** out, size_t bytes, hipStream_t stream) {
    const hipError_t e = allocate_block(out, bytes, stream);
    const int byte = poison_byte();
    if (e != hipSuccess || byte < 0) return e;
    const hipError_t filled = poison_lent(*out, bytes, stream, byte);
    if (filled != hipSuccess) {
        scratch_release(*out, stream);
        *out = nullptr;
    }
    return filled;
}

namespace {
hipError_t allocate_block(void** out, size_t bytes, hipStream_t stream) {
    int device = 0;
    if (!current_device(&device)) return hipMallocAsync(out, bytes, stream);
    ScratchState& state = scratch_state(device);
    const size_t want = ScratchLedger::block_size(bytes);
    if (stream_is_capturing(stream)) {
        hipMemPool_t pool = hip_pool(state, device);
        return pool != nullptr ? hipMallocFromPoolAsync(out, bytes, pool, stream) : hipMallocAsync(out, bytes, stream);
    }
    {
        std::unique_lock<std::mutex> lock(state.mutex);
        const size_t pick = state.ledger.match(want, stream);
        if (pick != ScratchLedger::kNone) {
            // The wait comes before the event can become a spare one: another thread could record it anew, and the wait
            // would order against the wrong point.  A failed wait leaves the block cached.
            const ScratchLedger::Block& block = state.ledger.cached()[pick];
            if (block.stream != stream) {
                const hipError_t e = hipStreamWaitEvent(stream, as_event(block.event), 0);
                if (e != hipSuccess) return e;
            }
            *out = state.ledger.take(pick);
            return hipSuccess;
        }
    }
    void* ptr = nullptr;
    {
        RelaxedCapture relaxed;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipErrorOutOfMemory) {  // the cache itself may be what fills the device
            (void)hipGetLastError();
            evict(state, 0);
            e = hipMalloc(&ptr, want);
        }
        if (e != hipSuccess) return e;
    }
    std::lock_guard<std::mutex> lock(state.mutex);
    state.ledger.lend(ptr, want);
    *out = ptr;
    return hipSuccess;
}
}  // namespace

void heamd::scratch_release(void* ptr, hipStream_t stream) {
    if (ptr == nullptr) return;
    if (poisoned_blocks().lent != 0) poison_released(ptr, stream);
    int device = 0;
    const bool known = current_device(&device);
    if (known && release_into(scratch_state(device), ptr, stream)) return;
    // a block of another device's cache (the caller changed the current device between the two ends of a call: the event is
    // then recorded on a stream of the block's own device, which `stream` is)
    for (int other = 0; other < kMaxDevices; ++other)
        if (!(known && other == device) && release_into(scratch_state(other), ptr, stream)) return;
    (void)hipFreeAsync(ptr, stream);  // from the HIP pool
}

extern "C" {

int he_set_scratch_cache(uint64_t bytes) {
    int device = 0;
    if (!current_device(&device)) {
        heamd::set_last_error("no current device");
        return HE_ERR_DEVICE;
    }
    ScratchState& state = scratch_state(device);
    {
        std::lock_guard<std::mutex> lock(state.mutex);
        state.limit = bytes;
    }
    evict(state, static_cast<size_t>(bytes));
    return HE_OK;
}
int he_device_trim_scratch(uint64_t keep_bytes) {
    int device = 0;
    if (!current_device(&device)) return HE_OK;
    ScratchState& state = scratch_state(device);
    evict(state, static_cast<size_t>(keep_bytes));
    RelaxedCapture relaxed;
    if (hipMemPool_t pool = state.pool) HEAMD_HIP_TRY(hipMemPoolTrimTo(pool, static_cast<size_t>(keep_bytes)));
    return HE_OK;
}
int he_scratch_cached_bytes(uint64_t* out_bytes) {
    if (out_bytes == nullptr) return invalid_argument("null out_bytes");
    *out_bytes = 0;
    int device = 0;
    if (!current_device(&device)) return HE_OK;
    ScratchState& state = scratch_state(device);
    std::lock_guard<std::mutex> lock(state.mutex);
    *out_bytes = state.ledger.cached_bytes();
    return HE_OK;
}

}  // extern "C"
