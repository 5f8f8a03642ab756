// sdma_route.h — library-internal: where an explicit-engine copy goes.
// Shared by sdma.hip (per-call resolution) and step.hip (resolved once per
// plan). Not part of the public hpk.h surface: it drags in the HSA headers.
#pragma once

#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <cstdint>

namespace hpk {
namespace detail {

struct SdmaRoute {
  hsa_agent_t dst_agent{};
  hsa_agent_t src_agent{};
  // one-hot hsa_amd_sdma_engine_id_t; 0 = no engine resolved (engine_index
  // < 0, or the status query reported none idle)
  uint32_t engine = 0;
};

// Owning agents of dst/src (two hsa_amd_pointer_info lookups) and the
// engine_index-th idle engine of that agent pair (one
// hsa_amd_memory_copy_engine_status query). Throws on a bad device index.
SdmaRoute sdma_resolve(const void* dst, const void* src, int device,
                       int engine_index);

// Throws std::runtime_error naming `what` unless s is HSA_STATUS_SUCCESS.
void check_hsa(hsa_status_t s, const char* what);

} // namespace detail
} // namespace hpk
