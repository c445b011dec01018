// The full-neighbour aggregations' launch constants and per-call prologue,
// shared by infer.hip (fp32 rows) and agghalf.hip (f16 feature rows): the
// item shapes, the hub switch, the hub list and the two degree-sqrt tables.
// Host side only.
#pragma once
#include "common.hpp"

namespace nts_hip {

constexpr int kInfThreads = 256;
constexpr int kInfU = 8;             // neighbour rows in flight per lane group
constexpr uint32_t kHubEdges = 2048; // rows longer than this are column-sliced
constexpr int kHubLpd = 16;          // lanes per hub item
constexpr uint32_t kHubGrid = 1024;  // hub kernel: grid-stride over the hub items

// The call's scratch (the two sqrt tables [V], the hub flags / their scan
// [n + 1], the hub list [n], the scan's temporaries) and the hub list of rows
// [v_begin, v_begin + n): flag, scan, scatter on the context's stream.
struct HubScratch {
  float *so, *si;
  uint32_t *pos, *hubs;  // pos[n] = the hub count
  float* extra;          // extra_words floats of the caller's own, 256-byte aligned
};
int list_hubs(nts_hip_ctx* ctx, const nts_graph_dev* graph, uint64_t v_begin, uint64_t n,
              HubScratch& h, size_t extra_words = 0);
// so[v] = degree_sqrt(out_degree[v]), si[v] = degree_sqrt(in_degree[v]) for every vertex
int degree_sqrt_tables(nts_hip_ctx* ctx, const nts_graph_dev* graph, float* so, float* si);

}  // namespace nts_hip
