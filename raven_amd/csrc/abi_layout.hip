// abi_layout.hip — C ABI (include/raven_hip.h): the force-directed layout (rvn_layout_force_directed).
#include <cmath>

#include "abi.h"

using namespace rvn;

extern "C" {

int rvn_layout_force_directed(rvn_engine* h, uint32_t n_components, const uint32_t* component_offsets, const double* xy_in,
                              const uint64_t* adj_offsets, const uint32_t* adj, uint32_t n_iterations, double* xy_out,
                              rvn_layout_stats* stats) {
  const bool args_ok = h && component_offsets && (n_components == 0 || (xy_in && adj_offsets && xy_out));
  return guarded(h, args_ok, "[raven_hip] rvn_layout_force_directed: NULL argument", [&](Engine& e) -> int {
    const char* who = "[raven_hip] rvn_layout_force_directed: ";
    if (stats) *stats = rvn_layout_stats{0, 0, 0};
    if (component_offsets[0] != 0) return fail(RVN_EINVAL, std::string(who) + "component_offsets must start at 0");
    for (u32 c = 0; c < n_components; ++c) {
      if (component_offsets[c + 1] < component_offsets[c]) return fail(RVN_EINVAL, std::string(who) + "component_offsets do not ascend");
      if (component_offsets[c + 1] == component_offsets[c])
        return fail(RVN_EINVAL, std::string(who) + "component " + std::to_string(c) + " is empty");
    }
    const u32 n = component_offsets[n_components];
    if (n > (1u << 28)) return fail(RVN_EINVAL, std::string(who) + "more than 2^28 points");
    if (n == 0) return RVN_OK;
    if (adj_offsets[0] != 0) return fail(RVN_EINVAL, std::string(who) + "adj_offsets must start at 0");
    for (u32 i = 0; i < n; ++i)
      if (adj_offsets[i + 1] < adj_offsets[i]) return fail(RVN_EINVAL, std::string(who) + "adj_offsets do not ascend");
    if (adj_offsets[n] && !adj) return fail(RVN_EINVAL, std::string(who) + "NULL argument");
    for (size_t i = 0; i < 2 * static_cast<size_t>(n); ++i)
      if (!std::isfinite(xy_in[i])) return fail(RVN_EINVAL, std::string(who) + "coordinate " + std::to_string(i) + " is not finite");
    for (u32 c = 0; c < n_components; ++c) {
      const u32 b = component_offsets[c], en = component_offsets[c + 1];
      for (u64 a = adj_offsets[b]; a < adj_offsets[en]; ++a)
        if (adj[a] < b || adj[a] >= en)
          return fail(RVN_EINVAL, std::string(who) + "neighbour " + std::to_string(adj[a]) + " is outside component " +
                                      std::to_string(c) + " of the point that lists it");
    }
    LayoutStats st;
    layout_force_directed(e, n_components, component_offsets, xy_in, adj_offsets, adj, n_iterations, xy_out, st);
    if (stats) *stats = rvn_layout_stats{st.host_tree_iterations, st.max_depth, 0};
    return RVN_OK;
  });
}

}  // extern "C"
