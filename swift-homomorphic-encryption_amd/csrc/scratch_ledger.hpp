// scratch_ledger.hpp -- the bookkeeping of the scratch block cache (scratch_cache.cpp).  Plain C++ (no HIP include): streams and
// events are opaque handles, a host compiler builds it, and tests/test_scratch_ledger.py holds its policy to a restatement in
// Python without a device.
//
// The ledger decides and performs nothing: it never allocates, frees, records, waits or queries.  Its owner asks under its
// mutex, acts on the answer, and reports the outcome back.  Not thread-safe by itself.
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace heamd {

class ScratchLedger {
  public:
    using Handle = void*;  // a stream or an event
    struct Block {
        void* ptr;
        size_t bytes;
        Handle stream;  // released on; forgotten() once that stream was destroyed
        Handle event;   // recorded on `stream` at the release; stays with the block for as long as the block is cached
        uint64_t tick;  // one per release, never reused: names THIS stay of the block in the cache
    };
    static constexpr size_t kNone = SIZE_MAX;

    // Requests are rounded up to 64 KiB below 1 MiB and to 1 MiB from there.
    static size_t block_size(size_t bytes) {
        const size_t grain = bytes >= (size_t(1) << 20) ? (size_t(1) << 20) : (size_t(64) << 10);
        return (bytes + grain - 1) / grain * grain;
    }
    // What no live stream compares equal to.
    static Handle forgotten() { return reinterpret_cast<Handle>(~uintptr_t(0)); }

    size_t cached_bytes() const { return cached_bytes_; }
    const std::vector<Block>& cached() const { return free_; }
    const std::map<void*, size_t>& lent() const { return lent_; }
    const std::vector<Handle>& spare_events() const { return spare_events_; }

    // The cached block a request of `want` bytes (a block_size) on `stream` takes, as an index into cached(), or kNone: the
    // smallest that holds the request without wasting more than half of itself; one released on this very stream first (it
    // needs no wait), then any other; among equals the earlier in the list.
    size_t match(size_t want, Handle stream) const {
        size_t pick = kNone;
        for (size_t i = 0; i < free_.size(); ++i) {
            const Block& b = free_[i];
            if (b.bytes < want || b.bytes > 2 * want) continue;
            if (pick == kNone) {
                pick = i;
                continue;
            }
            const Block& best = free_[pick];
            const bool same = b.stream == stream, best_same = best.stream == stream;
            if (same != best_same ? same : b.bytes < best.bytes) pick = i;
        }
        return pick;
    }
    // cached()[index] is lent out.  Its event becomes a spare one: whoever had to wait for it has done so.
    void* take(size_t index) {
        const Block block = remove(index);
        lent_[block.ptr] = block.bytes;
        return block.ptr;
    }
    // A block fresh from the driver is lent out.
    void lend(void* ptr, size_t bytes) { lent_[ptr] = bytes; }
    // A pointer comes back: its size, and it is the caller's from here on (to cache() or to free); 0: never lent by this ledger.
    size_t reclaim(void* ptr) {
        const auto it = lent_.find(ptr);
        if (it == lent_.end()) return 0;
        const size_t bytes = it->second;
        lent_.erase(it);
        return bytes;
    }
    // An event nobody uses, or nullptr (the caller creates one); and the way back for one that was not used after all.
    Handle take_spare_event() {
        if (spare_events_.empty()) return nullptr;
        const Handle event = spare_events_.back();
        spare_events_.pop_back();
        return event;
    }
    void give_spare_event(Handle event) { spare_events_.push_back(event); }
    // A reclaimed block joins the cache, released on `stream` where `event` was recorded behind its last use.
    void cache(void* ptr, size_t bytes, Handle stream, Handle event) {
        free_.push_back(Block{ptr, bytes, stream, event, ++tick_});
        cached_bytes_ += bytes;
    }
    // Takes blocks out of the cache until at most `keep` bytes stay: among those whose tick is in `completed` (the caller
    // queried each cached block's event once and names the stays whose release has finished), the oldest tick first.  Blocks
    // still in flight stay.  The victims, in order, are the caller's to free; their events are spare ones already.
    std::vector<Block> evict(size_t keep, const std::vector<uint64_t>& completed) {
        std::vector<Block> victims;
        while (cached_bytes_ > keep) {
            size_t pick = kNone;
            for (size_t i = 0; i < free_.size(); ++i) {
                bool done = false;
                for (const uint64_t tick : completed) done = done || tick == free_[i].tick;
                if (done && (pick == kNone || free_[i].tick < free_[pick].tick)) pick = i;
            }
            if (pick == kNone) break;
            victims.push_back(remove(pick));
        }
        return victims;
    }
    // A later stream may get the same handle: blocks released on this one no longer count as released on the requesting
    // stream (their events still order them).
    void forget_stream(Handle stream) {
        for (Block& block : free_)
            if (block.stream == stream) block.stream = forgotten();
    }

  private:
    // the one way out of the free list, and the one way an event of a block becomes spare
    Block remove(size_t index) {
        const Block block = free_[index];
        free_.erase(free_.begin() + static_cast<std::ptrdiff_t>(index));
        cached_bytes_ -= block.bytes;
        spare_events_.push_back(block.event);
        return block;
    }

    std::vector<Block> free_;
    std::map<void*, size_t> lent_;  // blocks of the cache that are in use -> their size
    std::vector<Handle> spare_events_;
    size_t cached_bytes_ = 0;
    uint64_t tick_ = 0;
};

}  // namespace heamd
