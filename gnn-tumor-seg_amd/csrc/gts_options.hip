// The option registry of the library (gts_set_option / gts_get_option): one table of option id, the knob it sets and
// the values it takes.  The knobs themselves live beside their kernels' shared code: gts_gemm_args.h (K11), gts_rows.h.
#include "gts_gemm_args.h"
#include "gts_rows.h"

namespace gts {
namespace {

struct Option { int32_t id; int* knob; bool (*legal)(int32_t); };   // legal == null: any value

const Option kOptions[] = {
    // the tile forms the library carries (the rejected ones live in tools/diag/gemm_rejected_forms.inc)
    {GTS_OPT_GEMM_TILE, &g_fwd_variant, [](int32_t v) { return v == -1 || v == -2 || v == 1 || v == 3 || v == 5 || v == 8 || v == 10; }},
    {GTS_OPT_IGRAD_TILE, &g_igrad_variant, [](int32_t v) { return v == -1 || v == 1 || v == 3 || v == 5 || v == 8 || v == 10; }},
    {GTS_OPT_WGRAD_TILE, &g_wgrad_variant, [](int32_t v) { return v == -1 || v == 1 || v == 2 || v == 4 || v == 6; }},
    {GTS_OPT_GEMM_SCHED, &g_gemm_sched, nullptr},
    {GTS_OPT_PANEL_ROWS, &g_panel_rows, nullptr},
    {GTS_OPT_SPMM_ROWS_PER_WAVE, &g_spmm_seq, nullptr},
    {GTS_OPT_SPMM_STREAMING, &g_spmm_nt, nullptr},
    {GTS_OPT_PROJECT_STREAMING, &g_project_nt, nullptr},
    {GTS_OPT_CLUSTER_STREAMING, &g_cluster_nt, nullptr},
    {GTS_OPT_CLUSTER_DEALING, &g_cluster_dealing, [](int32_t v) { return v >= 0 && v <= 2; }},
    {GTS_OPT_CLUSTER_RING, &g_cluster_ring, nullptr},
    {GTS_OPT_CLUSTER_PER_CU, &g_cluster_per_cu, nullptr},
    {GTS_OPT_CLUSTER_CONSUMERS, &g_cluster_consumers, nullptr},
    {GTS_OPT_GAT_WALK, &g_gat_walk, nullptr},
    {GTS_OPT_GAT_CLUSTER_WAVES, &g_gat_cluster_waves, nullptr},
    {GTS_OPT_GAT_CLUSTER_GROUP, &g_gat_cluster_group, nullptr},
    {GTS_OPT_GAT_CLUSTER_DEALING, &g_gat_cluster_dealing, [](int32_t v) { return v == 0 || v == 1; }},
};

const Option* find_option(int32_t id) {
  for (const Option& o : kOptions)
    if (o.id == id) return &o;
  return nullptr;
}

}  // namespace
}  // namespace gts

extern "C" int32_t gts_set_option(int32_t option, int32_t value) {
  const gts::Option* o = gts::find_option(option);
  if (o == nullptr || (o->legal != nullptr && !o->legal(value))) return GTS_ERR_ARGKIND;
  *o->knob = value;
  return GTS_OK;
}

extern "C" int32_t gts_get_option(int32_t option) {
  const gts::Option* o = gts::find_option(option);
  return o != nullptr ? *o->knob : INT32_MIN;
}
