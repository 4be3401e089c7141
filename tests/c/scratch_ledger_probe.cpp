// Drives csrc/scratch_ledger.hpp the way csrc/scratch_cache.cpp does, without a device, and prints every decision, for
// tests/test_scratch_ledger.py (a host program: the header includes nothing of HIP).
//
//   scratch_ledger_probe <script>
//
// One operation per line of the script, one line of output for each: the decision, " | ", the ledger's whole state.
// Pointers, streams and events are numbers the script makes up; a miss hands out the next "allocation", 0x10000 * count.
//   reset                           a fresh ledger, limit 0, no event complete               -> ok
//   limit <bytes>                   he_set_scratch_cache: sets the limit, evicts down to it  -> victims <ptr>...
//   request <bytes> <stream>        scratch_allocate                                         -> pool (limit 0: not the ledger's)
//                                                                                             | hit <ptr> wait=<0|1> | miss <ptr>
//   release <ptr> <stream> <event>  scratch_release; <event> is the one "created" should no spare one exist; the event used
//                                   is recorded anew (no longer complete); evicts down to the limit
//                                                                                            -> notmine | cached <event> victims <ptr>...
//   release_fail <ptr> <stream>     scratch_release whose event could not be recorded: the block is freed
//                                                                                            -> notmine | freed
//   complete <event>...             what was recorded on these events has finished           -> ok
//   evict <keep>                    he_device_trim_scratch                                   -> victims <ptr>...
//   forget <stream>                 scratch_forget_stream                                    -> ok
// State: cached=<bytes> free=[ptr:bytes:stream:event:tick ...] lent=[ptr:bytes ...] spare=[event ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "scratch_ledger.hpp"

using heamd::ScratchLedger;

namespace {
void* handle(uint64_t value) { return reinterpret_cast<void*>(static_cast<uintptr_t>(value)); }
uint64_t number(const void* h) { return static_cast<uint64_t>(reinterpret_cast<uintptr_t>(h)); }

struct Cache {
    ScratchLedger ledger;
    uint64_t limit = 0;
    uint64_t allocations = 0;
    std::set<void*> complete;  // events whose last record has finished

    // one pass: one answer per cached block, then the ledger's choice
    std::string evict(size_t keep) {
        std::vector<uint64_t> completed;
        if (ledger.cached_bytes() > keep)
            for (const ScratchLedger::Block& block : ledger.cached())
                if (complete.count(block.event) != 0) completed.push_back(block.tick);
        std::string out = "victims";
        for (const ScratchLedger::Block& block : ledger.evict(keep, completed)) out += " " + std::to_string(number(block.ptr));
        return out;
    }
    std::string state() const {
        std::ostringstream out;
        out << "cached=" << ledger.cached_bytes() << " free=[";
        const char* gap = "";
        for (const ScratchLedger::Block& b : ledger.cached()) {
            out << gap << number(b.ptr) << ":" << b.bytes << ":" << number(b.stream) << ":" << number(b.event) << ":" << b.tick;
            gap = " ";
        }
        out << "] lent=[";
        gap = "";
        for (const auto& entry : ledger.lent()) {
            out << gap << number(entry.first) << ":" << entry.second;
            gap = " ";
        }
        out << "] spare=[";
        gap = "";
        for (void* event : ledger.spare_events()) {
            out << gap << number(event);
            gap = " ";
        }
        out << "]";
        return out.str();
    }
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream script(argv[1]);
    if (!script) return 2;
    Cache* cache = new Cache();
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream words(line);
        std::string op;
        if (!(words >> op)) continue;
        std::vector<uint64_t> args;
        for (std::string word; words >> word;) args.push_back(std::strtoull(word.c_str(), nullptr, 0));
        std::string decision;
        if (op == "reset" && args.empty()) {
            delete cache;
            cache = new Cache();
            decision = "ok";
        } else if (op == "limit" && args.size() == 1) {
            cache->limit = args[0];
            decision = cache->evict(static_cast<size_t>(args[0]));
        } else if (op == "request" && args.size() == 2) {
            void* stream = handle(args[1]);
            const size_t want = ScratchLedger::block_size(static_cast<size_t>(args[0]));
            const size_t pick = cache->limit == 0 ? ScratchLedger::kNone : cache->ledger.match(want, stream);
            if (cache->limit == 0) {
                decision = "pool";
            } else if (pick != ScratchLedger::kNone) {
                const bool wait = cache->ledger.cached()[pick].stream != stream;
                decision = "hit " + std::to_string(number(cache->ledger.take(pick))) + (wait ? " wait=1" : " wait=0");
            } else {
                void* ptr = handle(++cache->allocations * 0x10000);
                cache->ledger.lend(ptr, want);
                decision = "miss " + std::to_string(number(ptr));
            }
        } else if ((op == "release" && args.size() == 3) || (op == "release_fail" && args.size() == 2)) {
            void* ptr = handle(args[0]);
            const size_t bytes = cache->ledger.reclaim(ptr);
            if (bytes == 0) {
                decision = "notmine";
            } else {
                void* event = cache->ledger.take_spare_event();
                if (op == "release_fail") {
                    if (event != nullptr) cache->ledger.give_spare_event(event);
                    decision = "freed";
                } else {
                    if (event == nullptr) event = handle(args[2]);
                    cache->complete.erase(event);
                    cache->ledger.cache(ptr, bytes, handle(args[1]), event);
                    decision = "cached " + std::to_string(number(event)) + " " + cache->evict(static_cast<size_t>(cache->limit));
                }
            }
        } else if (op == "complete") {
            for (const uint64_t event : args) cache->complete.insert(handle(event));
            decision = "ok";
        } else if (op == "evict" && args.size() == 1) {
            decision = cache->evict(static_cast<size_t>(args[0]));
        } else if (op == "forget" && args.size() == 1) {
            cache->ledger.forget_stream(handle(args[0]));
            decision = "ok";
        } else {
            std::fprintf(stderr, "bad operation: %s\n", line.c_str());
            return 2;
        }
        std::printf("%s | %s\n", decision.c_str(), cache->state().c_str());
    }
    delete cache;
    return 0;
}
