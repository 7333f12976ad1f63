// Host build of the fused pyramid's tile geometry (visual_sgraphs_amd/csrc/vsg_geometry.h) for tests/test_pyramid_seams.py
// and tests/test_gpu_pyramid_seams.py: the per-(tile, level) records k_pyramid reads and the seam-column helper it shares
// with the host.  Test-only, like tests/_hostcore.
#include <cstring>

#include "vsg_geometry.h"

using namespace vsg;

static Geometry g_geom;
static ExtractorTables g_tab;

extern "C" {

int ps_build(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, int rows, int cols) {
  if (!build_tables(g_tab, nfeatures, scaleFactor, nlevels, iniTh, minTh)) return -1;
  const uint16_t taps[7] = {18, 34, 49, 55, 49, 34, 18};
  return build_geometry(g_geom, g_tab, rows, cols, 0, 0, taps);
}
// {w, h, pitch, img_off} of level l
void ps_level(int l, int *out) {
  const LevelGeom &L = g_geom.fg.lv[l];
  out[0] = L.w, out[1] = L.h, out[2] = L.pitch, out[3] = L.img_off;
}
// {ntiles, lds bytes, ok, threads per tile, sizeof(PyrTileLevel)} of tiling i
void ps_tiling(int i, int *out) {
  const PyrTiling &P = g_geom.pyr[i];
  out[0] = (int)P.tiles.size(), out[1] = P.lds_bytes(), out[2] = P.ok, out[3] = kPyrThreads, out[4] = (int)sizeof(PyrTileLevel);
}
// record of (tiling i, tile t, level l): need[4], own[4], pitch, img_off, ncg, nrg, chunk, tab
void ps_tile_level(int i, int t, int l, int *out) {
  const PyrTileLevel &R = g_geom.pyr[i].tiles[t].lv[l];
  for (int k = 0; k < 4; k++) out[k] = R.need[k], out[4 + k] = R.own[k];
  out[8] = R.pitch, out[9] = R.img_off, out[10] = R.ncg, out[11] = R.nrg, out[12] = R.chunk, out[13] = R.tab;
}
// the helper itself: {a0, a1, nl, n} and the n seam columns of an owned column range [ox0, ox1); returns n
int ps_seam(int ox0, int ox1, int *desc, int *cols) {
  const PyrSeam S = pyr_seam(ox0, ox1);
  desc[0] = S.a0, desc[1] = S.a1, desc[2] = S.nl, desc[3] = S.n;
  for (int j = 0; j < S.n; j++) cols[j] = pyr_seam_column(S, ox0, j);
  return S.n;
}
}
