// workspace_layout.hpp -- where the parts of a call's workspace lie, stated once: a plan adds its parts in order and keeps the
// offsets it is given.  Plain C++ (no HIP include): tests/c/workspace_layout_probe.cpp holds it to Python's integers.
#pragma once

#include <cstddef>

namespace heamd {

inline size_t round16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

// Parts follow one another from byte 0, each rounded up to 16 bytes; an empty part shares its offset with the part behind it.
class WorkspaceLayout {
  public:
    size_t add(size_t bytes) {  // the offset of the new part
        const size_t offset = total_;
        total_ += round16(bytes);
        return offset;
    }
    size_t total() const { return total_; }

  private:
    size_t total_ = 0;
};

}  // namespace heamd
