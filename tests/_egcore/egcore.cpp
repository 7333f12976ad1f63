// The host build of csrc/vsg_essential_graph.h for the CPU tests: the whole of vsg_mappoints_optimize_essential_graph and
// vsg_mappoints_correct_sim3 with a caller array in the place of the store (the argument check is the library's own
// function), the pieces the tests measure on their own (dlog, lu3_solve, Sim3::log(), the edge error), and the edge-list
// builder of include/vsg_orb_adaptor.hpp.
#include "vsg_essential_graph.h"
#include "vsg_orb_adaptor.hpp"

using namespace vsg;

static thread_local std::vector<uint8_t> g_accepted;  // the last run's trials

extern "C" {

// the accept flag of every trial of the calling thread's last egcore_run, in order; returns their number
int egcore_last_trials(uint8_t *out, int cap) {
  for (size_t k = 0; k < g_accepted.size() && k < (size_t)cap; k++) out[k] = g_accepted[k];
  return (int)g_accepted.size();
}

// store_pos: [3 capacity] floats, read and written as the device call reads and writes the store (nullptr: no store)
int egcore_run(float *store_pos, int capacity, int n_kf, const vsg_sim3d *kf_Scw, const vsg_sim3d *kf_non_corrected,
               const uint8_t *kf_has_non_corrected, const uint8_t *kf_fixed, int n_edges, const int32_t *edge_i,
               const int32_t *edge_j, const uint8_t *edge_loop, int fix_scale, int iterations, int n_points, const int32_t *slots,
               const int32_t *point_ref, vsg_sim3d *kf_Scw_out, float *world_pos_out, double *chi2, vsg_essential_graph_result *res) {
  eg::HostRun R;
  int ran = 0;
  g_accepted.clear();
  const int rc = eg::check_and_build(n_kf, kf_Scw, kf_non_corrected, kf_has_non_corrected, kf_fixed, n_edges, edge_i, edge_j,
                                     edge_loop, fix_scale, iterations, n_points, slots, point_ref, store_pos ? capacity : -1,
                                     kf_Scw_out, res, &R.T, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    for (int k = 0; k < n_kf; k++) kf_Scw_out[k] = kf_Scw[k];
    eg::fill_result(res, R.T, nullptr);
    return VSG_OK;
  }
  std::vector<vsg_sim3d> nonc((size_t)n_kf);
  memset(nonc.data(), 0, nonc.size() * sizeof(vsg_sim3d));
  for (int k = 0; k < n_kf; k++)
    if (kf_has_non_corrected[k]) nonc[(size_t)k] = kf_non_corrected[k];
  R.setup(kf_Scw, nonc.data(), kf_has_non_corrected, fix_scale, iterations);
  R.run();
  g_accepted = R.accepted;
  R.outputs(kf_Scw, kf_Scw_out, chi2);
  std::vector<float> in(3 * (size_t)n_points), out(3 * (size_t)n_points);
  for (int i = 0; i < n_points; i++)
    for (int d = 0; d < 3; d++) in[3 * (size_t)i + d] = store_pos[3 * (size_t)slots[i] + d];
  R.correct(kf_Scw, n_points, point_ref, in.data(), out.data());
  for (int i = 0; i < n_points; i++)
    for (int d = 0; d < 3; d++) {
      store_pos[3 * (size_t)slots[i] + d] = out[3 * (size_t)i + d];
      if (world_pos_out) world_pos_out[3 * (size_t)i + d] = out[3 * (size_t)i + d];
    }
  eg::fill_result(res, R.T, &R.S);
  return VSG_OK;
}

int egcore_correct(float *store_pos, int capacity, int n_points, const int32_t *slots, const int32_t *point_ref, int n_ref,
                   const vsg_sim3d *S_from, const vsg_sim3d *S_to_inverse, float *world_pos_out) {
  if (!store_pos || n_points < 0 || n_ref < 0) return VSG_ERR_INVALID;
  if (n_points == 0) return VSG_OK;
  if (!S_from || !S_to_inverse || !eg::check_points(n_points, slots, point_ref, capacity, n_ref)) return VSG_ERR_INVALID;
  for (int r = 0; r < n_ref; r++)
    if (!eg::sim3_ok(S_from[r]) || !eg::sim3_ok(S_to_inverse[r])) return VSG_ERR_INVALID;
  for (int i = 0; i < n_points; i++) {
    float out[3];
    const int r = point_ref[i];
    eg::correct_point(sim3opt::sim3_of(S_from[r]), sim3opt::sim3_of(S_to_inverse[r]), store_pos + 3 * (size_t)slots[i], out);
    for (int d = 0; d < 3; d++) {
      store_pos[3 * (size_t)slots[i] + d] = out[d];
      if (world_pos_out) world_pos_out[3 * (size_t)i + d] = out[d];
    }
  }
  return VSG_OK;
}

void egcore_log(int n, const double *x, double *y) {
  for (int i = 0; i < n; i++) y[i] = eg::dlog(x[i]);
}
void egcore_lu3(const double *W, const double *t, double *x) {
  double M[3][3];
  for (int i = 0; i < 9; i++) M[i / 3][i % 3] = W[i];
  eg::lu3_solve(M, t, x);
}
void egcore_sim3_log(const vsg_sim3d *S, double *out7) { eg::sim3_log(sim3opt::sim3_of(*S), out7); }
void egcore_edge_error(const vsg_sim3d *C, const vsg_sim3d *v1, const vsg_sim3d *v2, double *out7) {
  eg::edge_error(sim3opt::sim3_of(*C), sim3opt::sim3_of(*v1), sim3opt::sim3_of(*v2), out7);
}

// vsg::essential_graph_edges on flat arrays; returns the number of edges (or -1: the adaptor threw), at most cap are written
int egcore_edges(int nKF, const int32_t *parent, const int32_t *loopOff, const int32_t *loopIdx, const int32_t *childOff,
                 const int32_t *childIdx, const int32_t *covOff, const int32_t *covIdx, int nLc, const int32_t *lcKf,
                 const int32_t *lcOff, const int32_t *lcIdx, const int32_t *lcWeight, int curKF, int loopKF, int cap, int32_t *ei,
                 int32_t *ej, uint8_t *eloop) {
  auto vec = [](const int32_t *p, size_t n) { return std::vector<int32_t>(p, p + n); };
  const size_t K = (size_t)nKF, M = (size_t)nLc;
  try {
    const EssentialGraphEdges E = essential_graph_edges(
        nKF, vec(parent, K), vec(loopOff, K + 1), vec(loopIdx, (size_t)loopOff[K]), vec(childOff, K + 1), vec(childIdx, (size_t)childOff[K]),
        vec(covOff, K + 1), vec(covIdx, (size_t)covOff[K]), vec(lcKf, M), vec(lcOff, M + 1), vec(lcIdx, (size_t)lcOff[M]),
        vec(lcWeight, (size_t)lcOff[M]), curKF, loopKF);
    for (size_t e = 0; e < E.i.size() && e < (size_t)cap; e++) ei[e] = E.i[e], ej[e] = E.j[e], eloop[e] = E.loop[e];
    return (int)E.i.size();
  } catch (const std::exception &) {
    return -1;
  }
}

}  // extern "C"
