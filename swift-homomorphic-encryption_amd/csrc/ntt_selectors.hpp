// ntt_selectors.hpp -- internal seam between the routing layer (ntt_routing.hip) and the kernel units: one selector per kernel
// family turns a butterfly mode into a kernel address and launches it.  Each is defined beside the kernel template it names
// (ntt_forward_tiled.hpp, ntt_inverse_tiled.hpp, ntt_interleaved.hpp) and explicitly instantiated, for the shapes the
// routing layer's templates refer to, in the unit that compiles those kernels (ntt_tiled_4096.hip, ntt_forward_8192.hip,
// ntt_inverse_8192.hip).  Three of them -- the tiled N = 16384 slab forms, forward and inverse -- sit behind branches the
// optimiser proves dead, so the optimised routing object does not name them; they are instantiated all the same, for an
// unoptimised build to link and because the single unit this was cut from instantiated them too.  The library is linked with --no-undefined (build.py), so a shape the routing layer gains without its
// instantiation fails the build, not the first call.
#pragma once

#include <hip/hip_runtime.h>

#include "device_context.hpp"
#include "ntt_rows.hpp"
#include "ntt_sources.hpp"

namespace heamd {

// ntt_forward_tiled.hpp
template <int LOGN, int LOGT, int SPREAD, int ROWS>
hipError_t launch_forward_kernel(int mode, uint64_t* slab, const DeviceContext& ctx, const ntt::RowMap& map, size_t workgroups,
                                 const ntt::SpreadSource& spread, hipStream_t stream);
// ntt_inverse_tiled.hpp
template <int LOGN, int LOGT, int SOURCE, int ROWS>
hipError_t launch_inverse_kernel(int mode, uint64_t* slab, const DeviceContext& ctx, const ntt::RowMap& map, size_t workgroups,
                                 const ntt::InverseSource& source_spec, hipStream_t stream);
// ntt_interleaved.hpp
template <int LOGS, int SPREAD>
hipError_t launch_interleaved_forward(int mode, uint64_t* slab, const DeviceContext& ctx, const ntt::RowMap& map, size_t rows,
                                      const ntt::SpreadSource& spread, hipStream_t stream);
template <int LOGS, int SOURCE>
hipError_t launch_interleaved_inverse(int mode, uint64_t* slab, const DeviceContext& ctx, const ntt::RowMap& map, size_t rows,
                                      const ntt::InverseSource& source_spec, hipStream_t stream);
// ntt_generic.hip: any power-of-two degree, rows <= 2^30
hipError_t launch_generic(bool inverse, uint64_t* slab, const DeviceContext& ctx, uint32_t mod_base, uint32_t mod_period, size_t rows,
                          hipStream_t stream);

}  // namespace heamd
