// zeroized_workspace.hpp -- the workspace of a call whose scratch depends on a secret or on a user's plaintext (encrypt_api.cpp:
// DRBG records, error polynomials, rotated keys; pnns_client_api.cpp: quantised queries, plaintexts, decrypted distances).
#pragma once

#include "api_internal.hpp"

namespace heamd {

// The workspace of one call: the caller's or stream-ordered scratch.  Its first `bytes` bytes are set to zero on the stream when
// the call is done with them, however it ends.
class ZeroizedWorkspace {
  public:
    explicit ZeroizedWorkspace(hipStream_t stream) : scratch_(stream), stream_(stream) {}
    ~ZeroizedWorkspace() {
        if (base_ != nullptr && bytes_ != 0 && hipMemsetAsync(base_, 0, bytes_, stream_) != hipSuccess) (void)hipGetLastError();
    }
    int resolve(void* workspace, size_t workspace_bytes, size_t needed) {
        if (workspace != nullptr) {
            if (workspace_bytes < needed) return invalid_argument("workspace too small");
            if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return invalid_argument("workspace not 16-byte aligned");
            base_ = static_cast<uint8_t*>(workspace);
        } else {
            HEAMD_HIP_TRY(scratch_.allocate(needed));
            base_ = static_cast<uint8_t*>(scratch_.get());
        }
        bytes_ = needed;
        return HE_OK;
    }
    template <typename T = uint8_t>  // the part at `offset` (a WorkspaceLayout's, workspace_layout.hpp) as words of T
    T* at(size_t offset) const { return reinterpret_cast<T*>(base_ + offset); }

  private:
    Scratch scratch_;  // (released after the destructor's memset: members go after the body)
    hipStream_t stream_;
    uint8_t* base_ = nullptr;
    size_t bytes_ = 0;
};

}  // namespace heamd
