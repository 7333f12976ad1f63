// fast_forms_host.cpp -- the product's host geometry (visual_sgraphs_amd/csrc/vsg_geometry.h) compiled for the CPU, for
// tests/test_gpu_fast_forms.py: the FastCellRec array of a geometry and what the host derives from it for launch_fast.
#include <cstring>

#include "vsg_geometry.h"

using namespace vsg;

static Geometry g_geom;
static ExtractorTables g_tab;

extern "C" {

int ff_build(int nfeatures, float scaleFactor, int nlevels, int iniTh, int minTh, int rows, int cols) {
  if (!build_tables(g_tab, nfeatures, scaleFactor, nlevels, iniTh, minTh)) return -1;
  const uint16_t taps[7] = {18, 34, 49, 55, 49, 34, 18};
  return build_geometry(g_geom, g_tab, rows, cols, 0, 0, taps);
}
// {cells, widest valid region, cand_segmented, plain as the geometry keeps it, tile pitch, prefetch chunks of the class}
void ff_info(int *out) {
  out[0] = g_geom.fg.total_cells, out[1] = g_geom.fastMaxVw, out[2] = g_geom.fg.cand_segmented;
  out[3] = g_geom.fastPlain ? 1 : 0, out[4] = fast_tile_pitch(g_geom.fastMaxVw);
  out[5] = fast_prefetch_chunks(out[4]);
}
// {x0, y0, x1, y1} of every cell's valid region (CellDesc), from which the records were derived
int ff_cells(int *out, int cap) {
  const int n = (int)g_geom.cells.size();
  for (int i = 0; i < n && i < cap; i++) {
    const CellDesc &c = g_geom.cells[i];
    out[4 * i] = c.x0, out[4 * i + 1] = c.y0, out[4 * i + 2] = c.x1, out[4 * i + 3] = c.y1;
  }
  return n;
}
// word 3 of every record, the one past the end included
int ff_w3(unsigned *out, int cap) {
  const int n = (int)g_geom.fastRecs.size();
  for (int i = 0; i < n && i < cap; i++) out[i] = g_geom.fastRecs[i].w[3];
  return n;
}
}
